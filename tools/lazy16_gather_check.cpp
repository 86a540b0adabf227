// lazy16_gather_check.cpp — a stand-alone host program over lazy16_gather (nns_internal.h), the per-lane gather that
// takes v_mfma_f32_16x16x32_bf16 operands out of an image written in the 32x32x16 operand order (OpLazySplit16,
// filter_mfma.hip).  No device is touched.  Build (host pass only):
//   hipcc --offload-arch=gfx950 --cuda-host-only -std=c++17 -Iinclude -Inns-cuda_amd/csrc tools/lazy16_gather_check.cpp -o lazy16_gather_check
// Checks, for every lane, both point tiles, all four k-steps, the hi and the lo part, in the ref layout (K2 form 3: one
// part's fragments back to back) and the query layout (form 2: hi | lo interleaved per 16-dim step):
//   * the 16 bytes the gather names hold the point and the dims that the 16x16x32 operand order wants at that lane —
//     order 1 of prep_kernels.hip (image_kernel<KT, 1>): lane l of fragment (tile, ks) = point 16 tile + (l & 15),
//     dims 32 ks + 8 (l >> 4) .. + 7 — given what the image holds there: fragment s, lane 32 hl + p = point p, dims
//     16 s + 8 hl .. + 7 (image_kernel<KT, 2 / 3>);
//   * the four k-steps of a tile together read every byte of the tile's half of the block exactly once;
//   * every ds_read_b128 lane group of the ring read covers the 64 LDS banks exactly once (conflict-free).
#include <stdio.h>
#include <set>
#include "nns_internal.h"

// what the image holds at 16-byte index idx of a block (parts = 1: form 3's hi or lo region, 2: form 2)
struct Held {
    int point, dim0, part;
};
static Held image_at(int idx, int parts)
{
    const int frag = idx / 64, lane = idx % 64;
    const int s = frag / parts;
    return {lane & 31, 16 * s + 8 * (lane >> 5), frag % parts};
}

int main()
{
    constexpr int KT = 128, NKS = KT / 32;
    int bad = 0;
    for (int parts = 1; parts <= 2; ++parts)
        for (int part = 0; part < parts; ++part)
            for (int t = 0; t < 2; ++t) {
                std::set<int> seen;
                for (int ks = 0; ks < NKS; ++ks)
                    for (int l = 0; l < 64; ++l) {
                        const int idx = nns::lazy16_gather(l, t, ks, parts, part);
                        const Held h = image_at(idx, parts);
                        // order 1: the operand the MFMA wants at lane l
                        const int want_point = 16 * t + (l & 15), want_dim0 = 32 * ks + 8 * (l >> 4);
                        if (idx < 0 || idx >= parts * (KT / 16) * 64 || h.point != want_point || h.dim0 != want_dim0 || h.part != part) {
                            printf("wrong bytes: parts %d part %d tile %d ks %d lane %d -> index %d = point %d dims %d.. part %d\n",
                                   parts, part, t, ks, l, idx, h.point, h.dim0, h.part);
                            ++bad;
                        }
                        if (!seen.insert(idx).second) {
                            printf("read twice: parts %d part %d tile %d index %d\n", parts, part, t, idx);
                            ++bad;
                        }
                    }
                if ((int)seen.size() != NKS * 64) ++bad;   // half of one part's KT / 16 fragments
            }
    // the ring read (ref hi fragments, parts = 1): ds_read_b128 is serviced in four groups of 16 lanes, banks
    // (byte address / 4) mod 64; a block starts at a multiple of 1 KiB, which does not move the banks
    static const int groups[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                      {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                      {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                      {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
    for (int t = 0; t < 2; ++t)
        for (int ks = 0; ks < NKS; ++ks)
            for (int gi = 0; gi < 4; ++gi) {
                std::set<int> banks;
                for (int e = 0; e < 16; ++e) {
                    const int byte = nns::lazy16_gather(groups[gi][e], t, ks) * 16;
                    for (int w = 0; w < 4; ++w) banks.insert((byte / 4 + w) % 64);
                }
                if (banks.size() != 64) {
                    printf("bank conflict: tile %d ks %d lane group %d covers %zu banks\n", t, ks, gi, banks.size());
                    ++bad;
                }
            }
    if (bad) return 1;
    printf("lazy16_gather ok: 2 layouts x hi / lo x 2 tiles x %d k-steps x 64 lanes; 32 lane groups on 64 banks each\n", NKS);
    return 0;
}
