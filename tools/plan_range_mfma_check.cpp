// plan_range_mfma_check.cpp — a stand-alone host program over the K7m planner (nns_plan_range_mfma, host only) and the
// threshold (nns_range_threshold), for a sanitizer build of the library's host code.  No device is touched.  Build from
// nns-cuda_amd/csrc, sources and this file into one program:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -I../../include -I. -Xarch_host -fsanitize=address,undefined \
//       ../../tools/plan_range_mfma_check.cpp *.hip -o plan_range_mfma_check -ldl -lpthread
// `plan_range_mfma_check dump` prints every field of the internal plan (range_mfma_plan: also what nns_plan_range_mfma
// does not export) over the grid of tests/test_range_mfma_cpu.py, one line per plan: the programs of two commits
// print the same text exactly when the planner is unchanged between them.
#include <stdio.h>
#include <string.h>
#include <math.h>
#include "nns_internal.h"

static int dump()
{
    const int ks[] = {8, 16, 17, 64, 128, 129, 256, 7, 257};
    const int ms[] = {64, 65, 513, 4096, 65536, 1 << 20};
    const int ns[] = {33, 1000, 70000, 1 << 20, 1 << 24};
    long plans = 0;
    for (int k : ks)
        for (int m : ms)
            for (int n : ns)
                for (int eager = 0; eager < 2; ++eager) {
                    nns::RangeMfmaPlan p{};
                    const int rc = nns::range_mfma_plan(k, m, n, eager != 0, &p);
                    printf("%d %d %d %d: rc %d kt %d spb %d qb %d qw %d n_pad %d total_slots %d blocks %d wpq %d lazy_img %d "
                           "batch %d batches %d flag_bytes %zu gx %d gy %d slots_per_split %d lds %d echunks %d eper %d "
                           "tiles %d offs_bytes %zu ws_bytes %zu\n",
                           k, m, n, eager, rc, p.kt, p.spb, p.qb, p.qw, p.n_pad, p.total_slots, p.blocks, p.wpq, p.lazy_img,
                           p.batch, p.batches, p.flag_bytes, p.gx, p.gy, p.slots_per_split, p.lds, p.echunks, p.eper, p.tiles,
                           p.offs_bytes, p.ws_bytes);
                    plans += rc == NNS_OK;
                }
    fprintf(stderr, "plans dumped %ld\n", plans);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "dump")) return dump();
    const int ks[] = {7, 8, 16, 17, 64, 128, 129, 256, 257};
    const int ms[] = {1, 64, 65, 513, 4096, 65536, 1 << 20, NNS_MAX_POINTS};
    const int ns[] = {1, 33, 1000, 70000, 1 << 20, 1 << 24, 1 << 27, NNS_MAX_POINTS};
    const unsigned fl[] = {0, NNS_FILTER_SPLIT_EAGER, NNS_FILTER_F32, NNS_FILTER_BF16};
    long ok = 0, unsupported = 0, bad = 0;
    for (int k : ks)
        for (int m : ms)
            for (int n : ns)
                for (unsigned f : fl) {
                    int out[10];
                    const int rc = nns_plan_range_mfma(k, m, n, f, out, 10);
                    if (rc == NNS_ERR_UNSUPPORTED) {
                        ++unsupported;
                        continue;
                    }
                    if (rc != NNS_OK) {
                        ++bad;
                        continue;
                    }
                    ++ok;
                    const long long blocks = out[2], batch = out[3], batches = out[4];
                    if (out[1] != 32 || blocks * 32 < n || batches * batch < m || (batches - 1) * batch >= m ||
                        out[5] <= 0 || out[5] > (256 << 20) || out[8] > 160 * 1024) {
                        printf("plan violates an invariant: k=%d m=%d n=%d flags=%u\n", k, m, n, f);
                        return 1;
                    }
                }
    float thr = 0;
    for (int kt = 16; kt <= 256; kt *= 2)
        for (float r2 : {0.0f, 1e-38f, 1.0f, 1e30f, 3.4e38f}) {
            if (nns_range_threshold(kt, 1.0f, 2.0f, r2, &thr) != NNS_OK || !(thr >= r2 - 1.0f)) {
                printf("threshold below the radius: kt=%d r2=%g thr=%g\n", kt, (double)r2, (double)thr);
                return 1;
            }
        }
    printf("plans ok %ld, unsupported %ld, invalid %ld\n", ok, unsupported, bad);
    return bad ? 1 : 0;
}
