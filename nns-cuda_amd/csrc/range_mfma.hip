// range_mfma.hip — K7m: the MFMA-filtered fixed-radius search (NNS_RANGE_MFMA; fp32 points on split-bf16 operands,
// bf16 points on exact operands).
//
// K7 evaluates V0's distance for every (query, ref) pair on the vector ALUs.  K7m asks the matrix cores first which
// 32-ref blocks can hold a hit at all, and evaluates V0 only there:
//   flag pass:  the eager split filter's tile (filter_mfma.hip, OpSplitT): refs are A and queries B of
//               v_mfma_f32_32x32x16_bf16, the accumulator seeded with |y'|^2, hi.hi + hi.lo + lo.hi per 16-dim step, a
//               wave's query operands resident, refs streamed through a 4-slot LDS ring by global_load_lds_dwordx4
//               with counted vmcnt waits and one barrier per slot.  K2's ref image is read in both layouts (eager:
//               hi, lo interleaved; lazy: hi region, lo region).  The threshold is FIXED per query before the loop
//               (range_threshold, nns_internal.h): no running minimum, no lists.  A finished 32 x 32 tile is tested
//               score by score with !(s > thr) — a NaN score passes — and a lane that passes sets the bit of
//               (its query, the 32-ref block) in the flag bitmap with a vector atomicOr (order-free: the bitmap is
//               deterministic; both lanes of a query set the same bit).
//   void rows:  a query with a non-finite coordinate or |v| >= 1e17 (the bound of K5's error model) gets its whole
//               flag row filled: the evaluation below is then the exact scan for it.
//   evaluation: one wave per (query, chunk of flag words) walks the words in ascending order; per set bit, lane = ref
//               of the block evaluates V0's chain (v0_lane_chains, the scan core of K7) on the ORIGINAL points and
//               applies K7's hit predicate.  Count writes per-(query, chunk) counts in K7's layout (K7's own kernels
//               turn them into lims); fill recomputes and writes each hit at chunk start + hits so far + ballot
//               prefix.  Blocks, lanes and chunks ascend: index order, no atomics, identical buffers every run.
//   bf16 points: the same ring, bitmap and evaluation; the tile is the 1-NN bf16 filter's (OpBF16T): K2's order-1
//               image, v_mfma_f32_16x16x32_bf16, ONE product per score (the operands are exact: no hi / lo, no
//               centring), threshold range_threshold(..., tau mode 1), 32 <= k <= 256.
//   uint8 points: the same ring, bitmap and evaluation; the tile is the int8 filter's (OpI8): K2's int8 image of the
//               values biased by 128, v_mfma_i32_16x16x64_i8, always at depth 256; the score is an exact integer and so
//               is the threshold (range_threshold_u8): a block is flagged if and only if it holds a hit.  32 <= k <= 256.
// The evaluation alone decides hits; a false flag costs time, never an answer.  Why no hit is missed: DESIGN §4 "K7m".
//
// Shared with the rest: the plan's geometry is filter_plan's (FilterGeom: fragment steps per block, query blocks per wave,
// waves and queries per workgroup, padding and ring slots — the one depth-to-operator table, filter_mfma.hip) and its
// ref-range splits are ring_pass_splits'; the workgroup and the ring slot are kSplitWaves / kSplitSlotSteps, which
// filter_mfma.hip asserts of the eager split operators; the hit predicate, the ballot prefix, kHuge and kWsBudget are
// nns_internal.h's.  The kernel's own: the ring loop below (same schedule as filter_main's, not the same code; one loop,
// range_flag_main, for both tile bodies), the fixed-threshold tile test, the bitmap and the evaluation.
#include "nns_internal.h"

namespace nns {

typedef float rm_f32x16 __attribute__((ext_vector_type(16)));
typedef float rm_f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 rm_bf16x8 __attribute__((ext_vector_type(8)));
typedef int rm_i32x4 __attribute__((ext_vector_type(4)));

constexpr int kRmWaves = kSplitWaves;                  // waves per workgroup: two per SIMD
constexpr int kRmSlotSteps = kSplitSlotSteps;          // 1 KiB fragments per ring slot
constexpr int kRmRing = 4;                             // ring slots
constexpr int kRmSlotCoord = kRmSlotSteps * 1024;
constexpr int kRmSlotBytes = kRmSlotCoord + 2048;      // + the slot's norms (up to 512 refs)
constexpr int kRmLds = kRmRing * kRmSlotBytes;
constexpr int kRmAhead = 3;                            // slots in flight ahead of the one being consumed
constexpr int kRmPpw = kRmSlotSteps / kRmWaves;        // image DMA pieces per wave and slot
constexpr int kRmEvalThreads = 256;
constexpr int kRmEvalWaves = kRmEvalThreads / 64;
constexpr int kRmBf16QB = kFlag16QB;                   // bf16 points: 32-query blocks per wave, at both depths

__device__ __forceinline__ rm_f32x16 rm_mma(const float4 &a, const float4 &b, rm_f32x16 acc)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(rm_bf16x8, a), __builtin_bit_cast(rm_bf16x8, b), acc, 0, 0,
                                                   0);
}

__device__ __forceinline__ rm_f32x4 rm_mma16(const float4 &a, const float4 &b, rm_f32x4 acc)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(rm_bf16x8, a), __builtin_bit_cast(rm_bf16x8, b), acc, 0, 0,
                                                   0);
}

__device__ __forceinline__ rm_i32x4 rm_mma8(const float4 &a, const float4 &b, rm_i32x4 acc)
{
    return __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(rm_i32x4, a), __builtin_bit_cast(rm_i32x4, b), acc, 0, 0, 0);
}

struct RangeFlagArgs {
    const float4 *qimg;     // the batch's query image (fp32 points: K2 form 2, qh, ql fragment per k-step; bf16 points:
                            // the order-1 image), [rows / 32][SPB][64]
    const char *rimg;       // K2's ref image
    const char *rimg_lo;    // lazy layout: the lo region; nullptr: the eager layout (and every bf16 image)
    const float *rnorm;     // [n_pad]
    const float *qnorm;     // the batch's squared norms (fp32 points: centred; bf16 points: as they are)
    const DevScalars *scal;
    unsigned *flags;        // [rows][wpq] words, bit b of a row = block b
    int rows_live;          // queries of the batch (rows beyond are padding: never flagged)
    int wpq;                // flag words per query
    int total_slots, slots_per_split, n_pad, kt;
    float radius2;
    const float *radius2v;  // per-query squared radii of the batch (K6m's bounds); nullptr: radius2 for every query
};

// ---- tile bodies: what a wave keeps resident, and what it does with one 32-ref block of a landed ring slot -------------
// load(): the wave's B operands, the lanes' fixed thresholds and flag rows; pin(): the loads are waited for before the
// ring starts (the compiler does not see the asm DMAs); block(): the scores of one block against the wave's queries,
// the test and the flag.  kt / 16 = SPB 1 KiB fragments per block and QB 32-query blocks per wave, either way.

// the threshold of query qi of the batch (tau mode MODE) and its flag row
// (padding rows: nothing passes !(s > -INF) but a NaN or -INF score, and their rows are never read.  A norm that is not
//  finite comes from a coordinate beyond 1e17, a per-query radius that is not finite from K6m's bound scan: that query's
//  row is filled behind this pass)
template <int MODE>
__device__ __forceinline__ float rm_lane_threshold(const RangeFlagArgs &a, int qi, float ymax2)
{
    const float qn = a.qnorm[qi];
    const bool live = qi < a.rows_live;
    const float r2 = a.radius2v && live ? a.radius2v[qi] : a.radius2;
    return live && qn < __builtin_inff() && r2 < __builtin_inff() ? range_threshold(a.kt, qn, ymax2, r2, MODE) : -__builtin_inff();
}

// fp32 points as split-bf16 operands (K2 form 2 / 3) on v_mfma_f32_32x32x16_bf16: hi, lo fragment per 16-dim step
template <int SPB, int QB>
struct RmSplitTile {
    static_assert(SPB >= 2 && SPB % 2 == 0, "hi / lo pairs");
    float4 bq[QB][SPB];
    float thr[QB];
    unsigned *row[QB];   // the flag row of the lane's query

    __device__ __forceinline__ void load(const RangeFlagArgs &a, int qblk0, int lane)
    {
        const float4 *src = a.qimg + (size_t)qblk0 * (SPB * 64) + lane;
        const float ymax2 = __uint_as_float(a.scal->ymax2_bits);
#pragma unroll
        for (int st = 0; st < QB; ++st) {
#pragma unroll
            for (int b = 0; b < SPB; ++b) bq[st][b] = src[(st * SPB + b) * 64];
            const int qi = (qblk0 + st) * 32 + (lane & 31);
            thr[st] = rm_lane_threshold<3>(a, qi, ymax2);
            row[st] = a.flags + (size_t)qi * a.wpq;
        }
    }
    __device__ __forceinline__ void pin()
    {
#pragma unroll
        for (int st = 0; st < QB; ++st) {
#pragma unroll
            for (int b = 0; b < SPB; ++b)
                asm volatile("" : "+v"(bq[st][b].x), "+v"(bq[st][b].y), "+v"(bq[st][b].z), "+v"(bq[st][b].w));
            asm volatile("" : "+v"(thr[st]));
        }
    }
    // slot: the ring slot; blk: the block within it; bg: the block's number = its bit in a flag row
    __device__ __forceinline__ void block(const char *slot, int blk, int bg, int lane) const
    {
        const int h = lane >> 5;
        rm_f32x16 acc0, acc1;
        // accumulators start at |y'_j|^2 of their rows: (r & 3) + 8 (r >> 2) + 4 h
        const float *nrm = reinterpret_cast<const float *>(slot + kRmSlotCoord) + blk * 32 + 4 * h;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 nv = *reinterpret_cast<const float4 *>(nrm + 8 * g);
            acc0[4 * g + 0] = nv.x;
            acc0[4 * g + 1] = nv.y;
            acc0[4 * g + 2] = nv.z;
            acc0[4 * g + 3] = nv.w;
        }
        acc1 = acc0;
        const float4 *fp = reinterpret_cast<const float4 *>(slot + blk * (SPB * 1024)) + lane;
#pragma unroll
        for (int b = 0; b < SPB; b += 2) {
            const float4 rh = fp[b * 64], rl = fp[(b + 1) * 64];
            // ref hi x (qh, ql) of the k-step, ref lo x qh
            acc0 = rm_mma(rh, bq[0][b], acc0);
            if constexpr (QB == 2) acc1 = rm_mma(rh, bq[1][b], acc1);
            acc0 = rm_mma(rh, bq[0][b + 1], acc0);
            if constexpr (QB == 2) acc1 = rm_mma(rh, bq[1][b + 1], acc1);
            acc0 = rm_mma(rl, bq[0][b], acc0);
            if constexpr (QB == 2) acc1 = rm_mma(rl, bq[1][b], acc1);
        }
#pragma unroll
        for (int st = 0; st < QB; ++st) {
            const rm_f32x16 t = st == 0 ? acc0 : acc1;
            bool pass = false;
#pragma unroll
            for (int r = 0; r < 16; ++r) pass = pass || !(t[r] > thr[st]);   // (a NaN score passes)
            if (__builtin_expect(__builtin_amdgcn_ballot_w64(pass) != 0ull, 0)) {   // rare, wave-uniform
                if (pass) atomicOr(row[st] + (bg >> 5), 1u << (bg & 31));
            }
        }
    }
};

// bf16 points, exact operands, on v_mfma_f32_16x16x32_bf16 over K2's order-1 image (prep_kernels.hip): fragment
// (kt / 32) t + ks of a 32-point block holds, at lane l, dims 32 ks + 8 (l >> 4) .. + 7 of point 16 t + (l & 15).  Refs
// are A, queries B; C lane l holds query column l & 15 and ref rows 4 (l >> 4) .. + 3.  The wave's 2 QB query tiles keep
// all their k-steps resident (2 QB kt / 32 fragments: 64 registers at kt = 128, 128 at kt = 256); per block, each of
// the two 16-ref tiles x 2 QB query tiles owns one accumulator, seeded with its four rows' norms.  Through the builtin:
// the compiler keeps the MFMA hazards.
template <int SPB, int QB>
struct RmBf16Tile {
    static constexpr int NKS = SPB / 2;   // 32-dim k-steps: kt / 32
    static constexpr int NQT = 2 * QB;    // 16-query tiles per wave
    static_assert(SPB == 8 || SPB == 16, "kt = 128 / 256: OpBF16K128 / OpBF16's blocks");
    float4 bq[NQT][NKS];
    float thr[NQT];
    unsigned *row[NQT];   // the flag row of the lane's query of tile qt: 16 qt + (lane & 15) of the wave's queries

    __device__ __forceinline__ void load(const RangeFlagArgs &a, int qblk0, int lane)
    {
        const float4 *src = a.qimg + (size_t)qblk0 * (SPB * 64) + lane;
        const float ymax2 = __uint_as_float(a.scal->ymax2_bits);
#pragma unroll
        for (int qt = 0; qt < NQT; ++qt) {
            // query block qt >> 1 of the wave, its point tile qt & 1
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) bq[qt][ks] = src[((qt >> 1) * SPB + (qt & 1) * NKS + ks) * 64];
            const int qi = qblk0 * 32 + 16 * qt + (lane & 15);
            thr[qt] = rm_lane_threshold<1>(a, qi, ymax2);
            row[qt] = a.flags + (size_t)qi * a.wpq;
        }
    }
    __device__ __forceinline__ void pin()
    {
#pragma unroll
        for (int qt = 0; qt < NQT; ++qt) {
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks)
                asm volatile("" : "+v"(bq[qt][ks].x), "+v"(bq[qt][ks].y), "+v"(bq[qt][ks].z), "+v"(bq[qt][ks].w));
            asm volatile("" : "+v"(thr[qt]));
        }
    }
    __device__ __forceinline__ void block(const char *slot, int blk, int bg, int lane) const
    {
        rm_f32x4 acc[2][NQT];
        // accumulators start at |y_j|^2 of their rows: 16 rt + 4 (lane >> 4) + 0 .. 3
        const float *nrm = reinterpret_cast<const float *>(slot + kRmSlotCoord) + blk * 32 + 4 * (lane >> 4);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
            const float4 nv = *reinterpret_cast<const float4 *>(nrm + 16 * rt);
#pragma unroll
            for (int qt = 0; qt < NQT; ++qt) acc[rt][qt] = rm_f32x4{nv.x, nv.y, nv.z, nv.w};
        }
        const float4 *fp = reinterpret_cast<const float4 *>(slot + blk * (SPB * 1024)) + lane;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const float4 r0 = fp[ks * 64], r1 = fp[(NKS + ks) * 64];
#pragma unroll
            for (int qt = 0; qt < NQT; ++qt) {
                acc[0][qt] = rm_mma16(r0, bq[qt][ks], acc[0][qt]);
                acc[1][qt] = rm_mma16(r1, bq[qt][ks], acc[1][qt]);
            }
        }
#pragma unroll
        for (int qt = 0; qt < NQT; ++qt) {
            bool pass = false;
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int e = 0; e < 4; ++e) pass = pass || !(acc[rt][qt][e] > thr[qt]);   // (a NaN score passes)
            // (the four lanes of a query, and both ref tiles, set the same bit)
            if (__builtin_expect(__builtin_amdgcn_ballot_w64(pass) != 0ull, 0)) {   // rare, wave-uniform
                if (pass) atomicOr(row[qt] + (bg >> 5), 1u << (bg & 31));
            }
        }
    }
};

// uint8 points on v_mfma_i32_16x16x64_i8 over K2's int8 image of the values biased by 128 (prep_kernels.hip,
// image_i8_kernel): fragment 4 t + ks of a 32-point block holds, at lane l, dims 64 ks + 16 (l >> 4) .. + 15 of point
// 16 t + (l & 15); always kt = 256, so SPB = 8 (OpI8's block: RmBf16Tile<8>'s bytes).  Refs are A, queries B; C lane l
// holds query column l & 15 and ref rows 4 (l >> 4) .. + 3.  Registers: the wave's 2 QB = 4 query tiles x 4 k-steps
// resident = 64 operand registers, 4 thresholds, 4 flag-row pointers (8); per block 2 x 4 i32 accumulators of 4 = 32,
// two ref fragments in flight = 8, the norms 8.  The accumulators start at the zero constant; after the fourth k-step an
// element becomes s = fma(-2, (float)acc, |y'|^2), exact as in OpI8::retire (|acc| <= 2^22, the norm an integer <= 2^22,
// |s| < 2^24), and is tested against the exact threshold (range_threshold_u8).  A padding ref's norm is +INF: s = +INF,
// never below a threshold.  Through the builtin: the compiler keeps the MFMA hazards.
template <int SPB, int QB>
struct RmU8Tile {
    static constexpr int NKS = SPB / 2;   // 64-dim k-steps: kt / 64
    static constexpr int NQT = 2 * QB;    // 16-query tiles per wave
    static_assert(SPB == 8, "kt = 256: OpI8's blocks");
    float4 bq[NQT][NKS];
    float thr[NQT];
    unsigned *row[NQT];   // the flag row of the lane's query of tile qt: 16 qt + (lane & 15) of the wave's queries

    __device__ __forceinline__ void load(const RangeFlagArgs &a, int qblk0, int lane)
    {
        const float4 *src = a.qimg + (size_t)qblk0 * (SPB * 64) + lane;
#pragma unroll
        for (int qt = 0; qt < NQT; ++qt) {
            // query block qt >> 1 of the wave, its point tile qt & 1
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) bq[qt][ks] = src[((qt >> 1) * SPB + (qt & 1) * NKS + ks) * 64];
            const int qi = qblk0 * 32 + 16 * qt + (lane & 15);
            // (padding rows and a per-query radius that is not finite: -INF, nothing passes; the latter's row is filled
            //  behind this pass)
            const bool live = qi < a.rows_live;
            const float r2 = a.radius2v && live ? a.radius2v[qi] : a.radius2;
            thr[qt] = live && r2 < __builtin_inff() ? range_threshold_u8(a.qnorm[qi], r2) : -__builtin_inff();
            row[qt] = a.flags + (size_t)qi * a.wpq;
        }
    }
    __device__ __forceinline__ void pin()
    {
#pragma unroll
        for (int qt = 0; qt < NQT; ++qt) {
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks)
                asm volatile("" : "+v"(bq[qt][ks].x), "+v"(bq[qt][ks].y), "+v"(bq[qt][ks].z), "+v"(bq[qt][ks].w));
            asm volatile("" : "+v"(thr[qt]));
        }
    }
    __device__ __forceinline__ void block(const char *slot, int blk, int bg, int lane) const
    {
        rm_i32x4 acc[2][NQT];
        const rm_i32x4 z = {0, 0, 0, 0};
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int qt = 0; qt < NQT; ++qt) acc[rt][qt] = z;
        const float4 *fp = reinterpret_cast<const float4 *>(slot + blk * (SPB * 1024)) + lane;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const float4 r0 = fp[ks * 64], r1 = fp[(NKS + ks) * 64];
#pragma unroll
            for (int qt = 0; qt < NQT; ++qt) {
                acc[0][qt] = rm_mma8(r0, bq[qt][ks], acc[0][qt]);
                acc[1][qt] = rm_mma8(r1, bq[qt][ks], acc[1][qt]);
            }
        }
        // |y'_j|^2 of the lane's rows: 16 rt + 4 (lane >> 4) + 0 .. 3
        const float *nrm = reinterpret_cast<const float *>(slot + kRmSlotCoord) + blk * 32 + 4 * (lane >> 4);
        const float4 n0 = *reinterpret_cast<const float4 *>(nrm), n1 = *reinterpret_cast<const float4 *>(nrm + 16);
        const float nv[2][4] = {{n0.x, n0.y, n0.z, n0.w}, {n1.x, n1.y, n1.z, n1.w}};
#pragma unroll
        for (int qt = 0; qt < NQT; ++qt) {
            bool pass = false;
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float s = __builtin_fmaf(-2.0f, (float)acc[rt][qt][e], nv[rt][e]);   // exact
                    pass = pass || !(s > thr[qt]);
                }
            // (the four lanes of a query, and both ref tiles, set the same bit)
            if (__builtin_expect(__builtin_amdgcn_ballot_w64(pass) != 0ull, 0)) {   // rare, wave-uniform
                if (pass) atomicOr(row[qt] + (bg >> 5), 1u << (bg & 31));
            }
        }
    }
};

// The flag pass of one workgroup: the ring over the refs of split blockIdx.y, TILE's body on every block of every slot.
// SPB: 1 KiB fragment steps per 32-ref block of K2's image (a ring slot is kRmSlotSteps of them, contiguous in the eager
// addressing); QB: 32-query blocks per wave
template <int SPB, int QB, class TILE>
__device__ __forceinline__ void range_flag_main(const RangeFlagArgs &a)
{
    constexpr int BPS = kRmSlotSteps / SPB;            // blocks per ring slot
    constexpr int SLOT_REFS = 32 * BPS;
    constexpr int NP = SLOT_REFS > 256 ? SLOT_REFS / 256 : 1;   // norm DMA pieces per slot
    static_assert(kRmSlotSteps % SPB == 0 && SPB >= 2, "whole blocks per slot");
    static_assert(SLOT_REFS * 4 <= kRmSlotBytes - kRmSlotCoord, "norm room of a ring slot");
    extern __shared__ __attribute__((aligned(16))) char rm_smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int qblk0 = (blockIdx.x * kRmWaves + wave) * QB;

    // ---- resident B operands and the lanes' fixed thresholds -------------------------------------------------
    TILE tile;
    tile.load(a, qblk0, lane);
    tile.pin();

    const int slot0 = blockIdx.y * a.slots_per_split;
    int ns = a.total_slots - slot0;
    if (ns > a.slots_per_split) ns = a.slots_per_split;
    const unsigned lds_base = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)rm_smem);

    // slot s (relative to slot0, s < ns: nothing is read past the image) into ring position s % kRmRing: the norms by
    // one wave, first, then every wave's kRmPpw image pieces — a counted wait that leaves the youngest slot's kRmPpw
    // pieces in flight has therefore seen every older piece land, norms included
    auto issue = [&](int s) __attribute__((always_inline)) {
        const size_t gslot = (size_t)(slot0 + s);
        const unsigned dst = lds_base + (s & (kRmRing - 1)) * kRmSlotBytes;
        if (((int)gslot & (kRmWaves - 1)) == wave) {
            if constexpr (SLOT_REFS >= 128) {
                // 256 norms per piece (a 128-ref slot: the upper lanes read the next slot's, or the array's last four)
#pragma unroll
                for (int np = 0; np < NP; ++np) {
                    size_t e = gslot * SLOT_REFS + np * 256 + lane * 4;
                    if (e > (size_t)a.n_pad - 4) e = (size_t)a.n_pad - 4;
                    dma16(a.rnorm + e, dst + kRmSlotCoord + np * 1024);
                }
            } else {
                size_t e = gslot * SLOT_REFS + lane;
                if (e > (size_t)a.n_pad - 1) e = (size_t)a.n_pad - 1;
                dma4(a.rnorm + e, dst + kRmSlotCoord);
            }
        }
#pragma unroll
        for (int p = 0; p < kRmPpw; ++p) {
            const int piece = wave * kRmPpw + p;
            if (a.rimg_lo) {
                // lazy layout: LDS fragment `piece` = block piece / SPB, k-step (piece % SPB) / 2, hi (even) or lo
                const int pb = piece / SPB, pf = piece % SPB;
                const char *reg = (pf & 1) ? a.rimg_lo : a.rimg;
                dma16(reg + ((gslot * BPS + pb) * (SPB / 2) + (pf >> 1)) * 1024 + lane * 16, dst + piece * 1024);
            } else {
                dma16(a.rimg + gslot * kRmSlotCoord + piece * 1024 + lane * 16, dst + piece * 1024);
            }
        }
    };

#pragma unroll
    for (int s = 0; s < kRmAhead; ++s)
        if (s < ns) issue(s);

    for (int s = 0; s < ns; ++s) {
        // slot s has landed: at most the pieces of the (up to two) younger slots stay in flight.  (vmcnt counts in issue
        // order; a flag atomic issued in between only makes the wait longer.)
        const int younger = ns - 1 - s;
        if (younger >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * kRmPpw) : "memory");
        else if (younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kRmPpw) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // everyone's share of slot s has landed; everyone is done with slot s - 1, whose ring position slot s + 3 takes
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if (s + kRmAhead < ns) issue(s + kRmAhead);
        const char *slot = rm_smem + (s & (kRmRing - 1)) * kRmSlotBytes;
#pragma unroll 1
        for (int blk = 0; blk < BPS; ++blk) tile.block(slot, blk, (slot0 + s) * BPS + blk, lane);
    }
}

// fp32 points: SPB = kt / 8 (hi, lo per 16-dim step)
template <int SPB, int QB>
__global__ __launch_bounds__(kRmWaves * 64) void range_flag_kernel(const RangeFlagArgs a)
{
    range_flag_main<SPB, QB, RmSplitTile<SPB, QB>>(a);
}

// bf16 points: SPB = kt / 16 — 8 (kt = 128, four blocks per ring slot) or 16 (kt = 256, two)
template <int SPB, int QB>
__global__ __launch_bounds__(kRmWaves * 64) void range_flag16_kernel(const RangeFlagArgs a)
{
    range_flag_main<SPB, QB, RmBf16Tile<SPB, QB>>(a);
}

// uint8 points: SPB = 8 (kt = 256 on 64-dim k-steps: four blocks per ring slot)
template <int SPB, int QB>
__global__ __launch_bounds__(kRmWaves * 64) void range_flag_u8_kernel(const RangeFlagArgs a)
{
    range_flag_main<SPB, QB, RmU8Tile<SPB, QB>>(a);
}

// one wave per query of the batch: a non-finite coordinate or |v| >= 1e17 — or, with per-query radii, a radius that is
// not finite — fills the query's flag row; filled (optional): += 1 per filled row
template <typename T>
__global__ __launch_bounds__(kRmEvalThreads) void range_void_rows_kernel(int k, int rows, const T *__restrict__ q,
                                                                         unsigned *__restrict__ flags, int wpq,
                                                                         const float *__restrict__ radius2v,
                                                                         unsigned long long *__restrict__ filled)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * kRmEvalWaves + (threadIdx.x >> 6);
    if (i >= rows) return;   // (whole waves)
    bool bad = false;
    for (int t = lane; t < k; t += 64) bad = bad || !(fabsf(pt_ld1(q + (size_t)i * k + t)) < kHuge);
    if (radius2v) bad = bad || !(radius2v[i] < __builtin_inff());
    if (__ballot(bad) == 0ull) return;
    for (int w = lane; w < wpq; w += 64) flags[(size_t)i * wpq + w] = 0xFFFFFFFFu;
    if (filled && lane == 0) atomicAdd(filled, 1ull);
}

// grid = (queries of the batch / waves per workgroup) x chunks.  One wave: query i0 + (its row), flag words
// [c * per, min((c + 1) * per, wpq)).  offs: [m][chunks] (several chunks): count writes the chunk's hits, fill reads the
// chunk's start within the query's segment.  lims: count writes lims[i + 1] (one chunk), fill reads lims[i], lims[i + 1].
// stat[0] (count): += the wave's flagged blocks that hold a ref below n.
template <int VEC, bool FILL, typename T>
__global__ __launch_bounds__(kRmEvalThreads) void range_eval_kernel(int k, int rows, int i0, int n, int per, int chunks,
                                                                    int wpq, float radius2, const T *__restrict__ q,
                                                                    const T *__restrict__ r,
                                                                    const unsigned *__restrict__ flags, int64_t index_base,
                                                                    int64_t *__restrict__ lims, int *__restrict__ offs,
                                                                    int *__restrict__ idx, float *__restrict__ dist,
                                                                    unsigned long long *__restrict__ stat)
{
    extern __shared__ __attribute__((aligned(16))) float rm_sq[];   // [waves][k]: each wave's query, widened to fp32
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * kRmEvalWaves + wave;
    if (row >= rows) return;   // (whole waves; no workgroup barrier below)
    const int64_t i = i0 + row;
    const int c = blockIdx.y;
    float *sq = rm_sq + (size_t)wave * k;
    for (int t = lane; t < k; t += 64) sq[t] = pt_ld1(q + (size_t)i * k + t);
    // (the wave reads only what it wrote itself: LDS operations of one wave complete in order)
    const unsigned *frow = flags + (size_t)row * wpq;
    const int w0 = c * per, w1 = w0 + per < wpq ? w0 + per : wpq;
    const int nblk = (n + 31) >> 5;   // blocks that hold a ref
    int64_t slot0 = 0, stop = 0;
    if (FILL) {
        slot0 = lims[i] + (chunks > 1 ? offs[(size_t)i * chunks + c] : 0);
        stop = lims[i + 1];
    }
    int run = 0;
    unsigned flagged = 0;
    for (int wb = w0; wb < w1; wb += 64) {
        const int w = wb + lane;
        unsigned word = w < w1 ? frow[w] : 0u;
        // (bits of blocks past the refs — a void row, padding blocks under an infinite threshold — are dropped)
        const int first = w << 5;
        if (first + 32 > nblk) word = first >= nblk ? 0u : word & (0xFFFFFFFFu >> (first + 32 - nblk));
        flagged += __popc(word);
        uint64_t live = __ballot(word != 0u);
        while (live) {   // wave-uniform: the non-empty words of this step, ascending
            const int src = __builtin_ctzll(live);
            live &= live - 1;
            unsigned bits = (unsigned)__shfl((int)word, src);
            const int blk0 = (wb + src) << 5;
            while (bits) {   // two set bits per round: the lower block on lanes 0 - 31, the next on lanes 32 - 63
                const int b0 = __builtin_ctz(bits);
                bits &= bits - 1;
                int b1 = -1;
                if (bits) {
                    b1 = __builtin_ctz(bits);
                    bits &= bits - 1;
                }
                const int b = lane < 32 ? b0 : b1;
                const int64_t j = ((int64_t)(blk0 + b) << 5) + (lane & 31);
                float sum[1] = {__builtin_nanf("")};   // a lane without a ref hits nothing
                if (b >= 0 && j < n) v0_lane_chains<1, VEC, 8>(k, sq, r + (size_t)j * k, sum);
                const bool hit = range_hit(sum[0], radius2);
                const uint64_t mask = __ballot(hit);
                if (FILL) {
                    const int64_t slot = slot0 + run + lanes_below(mask);
                    // (slot < stop holds whenever the points are those the count saw; the bound keeps a fill after
                    //  the caller changed them inside the buffers)
                    if (hit && slot < stop) {
                        if (idx) idx[slot] = (int)(index_base + j);
                        if (dist) dist[slot] = sum[0];
                    }
                }
                run += __popcll(mask);
            }
        }
    }
    if (FILL) return;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) flagged += __shfl_xor((int)flagged, d);
    if (lane == 0) {
        if (chunks > 1) offs[(size_t)i * chunks + c] = run;
        else lims[i + 1] = run;
        if (flagged) atomicAdd(stat, (unsigned long long)flagged);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------
// The flag kernels of bf16 points keep OpBF16K128 / OpBF16's geometry (filter_mfma.hip): 8 or 16 fragments per block, two
// query blocks per wave (64 / 128 resident operand registers, no scratch), the split operators' workgroup and ring slot
static_assert(kRmBf16QB * kRmWaves * 32 == 512, "filter_plan's queries per workgroup at the 16x16x32 depths");

int range_mfma_plan(int k, int m, int n, bool split_eager, RangeMfmaPlan *p, int dtype)
{
    const PointType &pt = point_type(dtype);
    if ((unsigned)dtype >= DT_COUNT || !pt.flag_kmax) {   // (a code the ABI does not define has no flag pass either)
        set_error("the range-MFMA flag: no flag pass for point dtype %d", dtype);
        return NNS_ERR_UNSUPPORTED;
    }
    const bool bf16 = dt_bf16_like(dtype), u8 = dtype == DT_U8;   // (uint8 points: the int8 tile's geometry = the 128-deep bf16 one)
    if (k <= 0 || m <= 0 || n <= 0) return NNS_ERR_INVALID;
    if (k < pt.flag_kmin || k > pt.flag_kmax) {
        set_error(bf16 ? "the range-MFMA flag: k = %d outside 32 .. 256 (bf16 and uint8 points: the 16x16 tiles)"
                       : "the range-MFMA flag: k = %d outside 8 .. 256 (the split-bf16 tiles)", k);
        return NNS_ERR_UNSUPPORTED;
    }
    FilterGeom g{};
    FilterRequest rq{};
    rq.k = k, rq.m = m, rq.n = n, rq.dtype = dtype, rq.form = pt.filter_form, rq.split_eager = split_eager;
    NNS_TRY(filter_plan(rq, &g));
    // (the form asked for must be the one granted; the 16x16 flag kernels: OpBF16K128 / OpBF16's geometry, uint8 the former's)
    if (g.form != rq.form ||
        (bf16 && (g.lpq != 4 || g.qb != kRmBf16QB || g.waves != kRmWaves || (g.spb != 8 && (u8 || g.spb != 16))))) {
        set_error("the range-MFMA flag: no %s tile for k = %d", u8 ? "16x16x64 int8" : bf16 ? "16x16x32 bf16" : "split-bf16", k);
        return NNS_ERR_UNSUPPORTED;
    }
    p->dtype = dtype;
    p->kt = g.kt;
    p->spb = g.spb;
    p->qb = g.qb;
    p->qw = g.qw;
    p->n_pad = g.n_pad;
    p->total_slots = g.total_slots;
    p->blocks = g.n_pad / 32;
    p->wpq = divup(p->blocks, 32);
    p->lazy_img = g.lazy_img;
    p->lds = kRmLds;
    // query batches: whole workgroups' worth of rows within the bitmap's cap
    const size_t row_bytes = (size_t)p->wpq * sizeof(unsigned);
    const int64_t cap_rows = (int64_t)(kWsBudget / row_bytes) / p->qw * p->qw;
    if (cap_rows < p->qw) {
        set_error("the range-MFMA flag: n = %d: one workgroup's flag rows exceed the 256 MiB workspace", n);
        return NNS_ERR_UNSUPPORTED;
    }
    const int64_t m_pad = (int64_t)divup(m, p->qw) * p->qw;
    p->batch = (int)(m_pad < cap_rows ? m_pad : cap_rows);
    p->batches = divup(m, p->batch);
    p->flag_bytes = (size_t)p->batch * row_bytes;
    p->gx = p->batch / p->qw;
    p->slots_per_split = divup(p->total_slots, ring_pass_splits(p->gx, p->total_slots));
    p->gy = divup(p->total_slots, p->slots_per_split);
    // evaluation: chunks of whole 64-word steps, about 4096 waves
    int64_t chunks = divup(4096, m);
    const int steps = divup(p->wpq, kRmChunkWords);
    if (chunks > steps) chunks = steps;
    // (K7's workspace rule: [m][chunks] counts within the range workspace's cap)
    const int64_t by_ws = (int64_t)(kWsBudget / ((size_t)m * sizeof(int)));
    if (chunks > by_ws) chunks = by_ws;
    if (chunks > 65535) chunks = 65535;
    if (chunks < 1) chunks = 1;
    p->eper = divup(steps, (int)chunks) * kRmChunkWords;
    p->echunks = divup(p->wpq, p->eper);
    p->tiles = range_scan_tiles(m);
    p->offs_bytes = p->echunks > 1 ? ((size_t)m * p->echunks * sizeof(int) + 7) & ~(size_t)7 : 0;
    p->ws_bytes = p->offs_bytes + (p->tiles > 1 ? (size_t)p->tiles * sizeof(int64_t) : 0);
    return NNS_OK;
}

template <int SPB, int QB>
static int launch_flag_t(const RangeMfmaPlan &p, const RangeFlagArgs &a, int gx, hipStream_t st)
{
    return launch_lds(range_flag_kernel<SPB, QB>, dim3(gx, p.gy), dim3(kRmWaves * 64), (size_t)kRmLds, st, a);
}
template <int SPB>
static int launch_flag16_t(const RangeMfmaPlan &p, const RangeFlagArgs &a, int gx, hipStream_t st)
{
    return launch_lds(range_flag16_kernel<SPB, kRmBf16QB>, dim3(gx, p.gy), dim3(kRmWaves * 64), (size_t)kRmLds, st, a);
}

// the flag pass of one query batch: rows [i0, i0 + rows) of the prepared query image / norms; the bitmap is zeroed on
// the stream first, void queries' rows are filled behind the pass
int launch_range_flags(const RangeMfmaPlan &p, int k, int i0, int rows, const void *q, const void *qimg, const float *qnorm,
                       const void *rimg, const float *rnorm, const DevScalars *scal, float radius2, void *flags,
                       hipStream_t st, const float *radius2v, unsigned long long *filled)
{
    const int rows_pad = divup(rows, p.qw) * p.qw;
    if (i0 % p.qw != 0 || rows_pad > p.batch) return NNS_ERR_INVALID;
    NNS_HIP(hipMemsetAsync(flags, 0, (size_t)rows_pad * p.wpq * sizeof(unsigned), st));
    RangeFlagArgs a;
    a.qimg = reinterpret_cast<const float4 *>(qimg) + (size_t)(i0 / 32) * (p.spb * 64);
    a.rimg = reinterpret_cast<const char *>(rimg);
    a.rimg_lo = p.lazy_img ? a.rimg + (size_t)p.n_pad * p.kt * 2 : nullptr;
    a.rnorm = rnorm;
    a.qnorm = qnorm + i0;
    a.scal = scal;
    a.flags = reinterpret_cast<unsigned *>(flags);
    a.rows_live = rows;
    a.wpq = p.wpq;
    a.total_slots = p.total_slots;
    a.slots_per_split = p.slots_per_split;
    a.n_pad = p.n_pad;
    a.kt = p.kt;
    a.radius2 = radius2;
    a.radius2v = radius2v;
    const int gx = rows_pad / p.qw;
    // (spb, qb) of the two 16x16x32 bf16 operators, of the five eager split operators
    const auto is = [&p](int spb, int qb) { return p.spb == spb && p.qb == qb; };
    if (p.dtype == DT_U8) {
        if (!is(8, kRmBf16QB) || p.kt != 256) {
            set_error("the range-MFMA flag: no uint8 flag kernel for %d fragment steps per block, %d query blocks per wave", p.spb, p.qb);
            return NNS_ERR_UNSUPPORTED;
        }
        NNS_TRY(launch_lds(range_flag_u8_kernel<8, kRmBf16QB>, dim3(gx, p.gy), dim3(kRmWaves * 64), (size_t)kRmLds, st, a));
    } else if (p.dtype == DT_BF16 && is(8, kRmBf16QB)) NNS_TRY((launch_flag16_t<8>(p, a, gx, st)));
    else if (p.dtype == DT_BF16 && is(16, kRmBf16QB)) NNS_TRY((launch_flag16_t<16>(p, a, gx, st)));
    else if (p.dtype == DT_BF16) {
        set_error("the range-MFMA flag: no bf16 flag kernel for %d fragment steps per block, %d query blocks per wave", p.spb, p.qb);
        return NNS_ERR_UNSUPPORTED;
    } else if (is(2, 2)) NNS_TRY((launch_flag_t<2, 2>(p, a, gx, st)));
    else if (is(4, 2)) NNS_TRY((launch_flag_t<4, 2>(p, a, gx, st)));
    else if (is(8, 2)) NNS_TRY((launch_flag_t<8, 2>(p, a, gx, st)));
    else if (is(16, 2)) NNS_TRY((launch_flag_t<16, 2>(p, a, gx, st)));
    else if (is(32, 1)) NNS_TRY((launch_flag_t<32, 1>(p, a, gx, st)));
    else {
        set_error("the range-MFMA flag: no flag kernel for %d fragment steps per block, %d query blocks per wave", p.spb, p.qb);
        return NNS_ERR_UNSUPPORTED;
    }
    if (p.dtype == DT_U8)   // (no uint8 value voids a row: only a per-query radius that is not finite fills one)
        hipLaunchKernelGGL(range_void_rows_kernel<u8_t>, dim3(divup(rows, kRmEvalWaves)), dim3(kRmEvalThreads), 0, st, k,
                           rows, (const u8_t *)q + (size_t)i0 * k, reinterpret_cast<unsigned *>(flags), p.wpq, radius2v,
                           filled);
    else if (p.dtype == DT_BF16)
        hipLaunchKernelGGL(range_void_rows_kernel<uint16_t>, dim3(divup(rows, kRmEvalWaves)), dim3(kRmEvalThreads), 0, st, k,
                           rows, (const uint16_t *)q + (size_t)i0 * k, reinterpret_cast<unsigned *>(flags), p.wpq, radius2v,
                           filled);
    else
        hipLaunchKernelGGL(range_void_rows_kernel<float>, dim3(divup(rows, kRmEvalWaves)), dim3(kRmEvalThreads), 0, st, k, rows,
                           (const float *)q + (size_t)i0 * k, reinterpret_cast<unsigned *>(flags), p.wpq, radius2v, filled);
    NNS_HIP(hipGetLastError());
    return NNS_OK;
}

// the evaluation of one query batch (fill: idx / dist; count: the per-(query, chunk) counts and stat[0])
template <typename T>
static int launch_range_eval_t(const RangeMfmaPlan &p, bool fill, int k, int i0, int rows, int n, const T *q, const T *r,
                               const void *flags, float radius2, int64_t base, int64_t *lims, void *ws, int *idx,
                               float *dist, unsigned long long *stat, hipStream_t st)
{
    int *offs = p.echunks > 1 ? (int *)ws : nullptr;
    // (K7's rule: four values of a row per load where the rows are 16- (fp32) / 8-byte (bf16) / 4-byte (uint8) aligned)
    const bool vec = (k % 4 == 0) && (((uintptr_t)r & (4 * sizeof(T) - 1)) == 0);
    const dim3 grid(divup(rows, kRmEvalWaves), p.echunks);
    const size_t lds = (size_t)kRmEvalWaves * k * sizeof(float);
    auto go = [&](auto kern) {
        return launch_lds(kern, grid, dim3(kRmEvalThreads), lds, st, k, rows, i0, n, p.eper, p.echunks, p.wpq, radius2, q, r,
                          (const unsigned *)flags, base, lims, offs, idx, dist, stat);
    };
    if (fill) return vec ? go(range_eval_kernel<4, true, T>) : go(range_eval_kernel<1, true, T>);
    return vec ? go(range_eval_kernel<4, false, T>) : go(range_eval_kernel<1, false, T>);
}

int launch_range_eval(const RangeMfmaPlan &p, bool fill, int k, int i0, int rows, int n, const void *q, const void *r,
                      const void *flags, float radius2, int64_t base, int64_t *lims, void *ws, int *idx, float *dist,
                      unsigned long long *stat, hipStream_t st)
{
    if (p.dtype == DT_U8)
        return launch_range_eval_t(p, fill, k, i0, rows, n, (const u8_t *)q, (const u8_t *)r, flags, radius2, base, lims, ws,
                                   idx, dist, stat, st);
    if (p.dtype == DT_BF16)
        return launch_range_eval_t(p, fill, k, i0, rows, n, (const uint16_t *)q, (const uint16_t *)r, flags, radius2, base,
                                   lims, ws, idx, dist, stat, st);
    return launch_range_eval_t(p, fill, k, i0, rows, n, (const float *)q, (const float *)r, flags, radius2, base, lims, ws,
                               idx, dist, stat, st);
}

}  // namespace nns
