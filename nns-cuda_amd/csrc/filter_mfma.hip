// filter_mfma.hip — K3 (fp32) / K4 (bf16): the MFMA filter.  The dominant kernel.
//
// What the reference does here: V1/V2 write the full m x n distance matrix
// (get_dis_kernel, core.cu:58-78) and reduce its rows (get_min_kernel core.cu:87-122 /
// thrust::min_element core.cu:197-198); V3-V9 fuse the two but give one 1024-thread
// block to each query and re-stream every reference point per query
// (core.cu:589-633).  At 65536 x 1048576 x 128 the matrix would be 256 GiB.
//
// What this kernel does instead: the ||q - r||^2 expansion.  With x' = q - c, y' = r - c
// (centred by K2; c = 0 on the bf16 path),
//     s(i, j) = |y'_j|^2 - 2 x'_i . y'_j            ( = ||q_i - r_j||^2 - |x'_i|^2 )
// has the same argmin over j.  -2 * Y' * X'^T is a dense GEMM on the matrix cores
// (v_mfma_f32_32x32x2_f32: exact fp32 FMA chain; v_mfma_f32_16x16x32_bf16: bf16 inputs,
// fp32 accumulate) with |y'_j|^2 preloaded as the accumulator's initial value, so the
// finished accumulator IS s(i, j) and the matrix never leaves the registers.
//
// Fused epilogue = RECORD COLLECTION, not a plain argmin: a lane keeps the running
// minimum m1 of its query over the refs it has seen and a threshold
// thr = m1 + tau(m1), where tau bounds |s + |x'|^2 - V0's fp32 distance| from both sides
// (derivation in finalize.hip).  Per 32x32 tile it takes the minimum of its 16 scores
// (8 v_min3 + 1 v_cmp); only when that beats thr (a new record or a near-record: about
// ln(n) times per lane in total) does a wave-uniform slow path append (score, index)
// entries to the lane's private candidate list in HBM.  Every ref whose score is within
// tau of the query's final minimum is therefore in some list, and K5 re-ranks exactly
// those few candidates with V0's own arithmetic: indices come out bit-identical to V0
// although the filter itself is approximate.
//
// Geometry (fp32; what the bf16 instantiation does differently is described at OpBF16T):
//   * MFMA A = refs (rows of the 32x32 tile), B = queries (columns): the C layout puts
//     a query on a lane (col = lane & 31) and 16 refs in the lane's 16 accumulator
//     registers, so the running state is per lane and needs no cross-lane traffic.
//   * a wave owns 64 queries (two blocks of 32; one block at the 256-deep tile); their B
//     operands for all of K (128 VGPRs) are loaded once and stay resident.  A workgroup is
//     8 waves = 512 queries; all 8 waves consume the same stream of ref blocks from LDS (a
//     block fetched once feeds 512 queries; the reference's V7 re-reads it per query).
//   * refs stream through a 4-slot LDS ring (slot = 64 refs = 32 KiB of K2's tile image
//     + 256 B of norms) filled by LDS-DMA (global_load_lds_dwordx4: the image is stored in
//     LDS order, so the copy is linear, 1 KiB per wave-instruction), waited for with
//     vmcnt and ONE raw s_barrier per slot; A fragments are lane-linear ds_read_b128
//     (bank-conflict free by construction of the image).
//   * the two waves that share a SIMD (w and w + 4) run HALF A BLOCK out of phase: waves
//     4..7 lag by half a 32-ref block (they finish the previous slot's last half block
//     after the barrier), so one partner's epilogue / accumulator re-seed / LDS latency
//     falls in the middle of the other's MFMA chain instead of both stalling together
//     at every block boundary (MI355X guide, "Two waves per SIMD", item 9).
//   * grid = (m_pad / 512) x splits; the split count minimises rounds x work per
//     workgroup (one resident workgroup per CU), see filter_plan.
//
// Roofline: MFMA-bound.  fp32: 64 MFMAs x 64 cycles per 32x32x128 tile per SIMD; bf16:
// 32 MFMAs x 16 cycles per 32x32x256 tile (four 16x16 tiles x 8 k-steps).  Algorithmic HBM
// traffic = the images once.
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <atomic>
#include <type_traits>
#include <vector>
#include "nns_internal.h"

namespace nns {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// compile-time unrolled loop: f(integral_constant<int, 0>) ... f(integral_constant<int, N-1>)
template <int N, int I = 0, class F>
__device__ __forceinline__ void static_for(F &&f)
{
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<N, I + 1>(f);
    }
}

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// accumulators of a wave's query blocks as NAMED members (an array of ext-vectors passed by
// reference is not scalarised by hipcc and lands in scratch)
struct AccSet {
    f32x16 v0, v1;
    template <int I>
    __device__ __forceinline__ f32x16 &at()
    {
        if constexpr (I == 0) return v0;
        else return v1;
    }
    template <int I>
    __device__ __forceinline__ const f32x16 &at() const
    {
        if constexpr (I == 0) return v0;
        else return v1;
    }
};

// The same 32 registers as eight 16x16 tiles [ref tile rt][query tile qt] (OpBF16T)
typedef float f32x4 __attribute__((ext_vector_type(4)));
struct AccSet16 {
    f32x4 t00, t01, t02, t03, t10, t11, t12, t13;
    template <int RT, int QT>
    __device__ __forceinline__ f32x4 &at()
    {
        static_assert(RT >= 0 && RT < 2 && QT >= 0 && QT < 4, "2 ref tiles x 4 query tiles");
        if constexpr (RT == 0) {
            if constexpr (QT == 0) return t00;
            else if constexpr (QT == 1) return t01;
            else if constexpr (QT == 2) return t02;
            else return t03;
        } else {
            if constexpr (QT == 0) return t10;
            else if constexpr (QT == 1) return t11;
            else if constexpr (QT == 2) return t12;
            else return t13;
        }
    }
    template <int RT, int QT>
    __device__ __forceinline__ const f32x4 &at() const
    {
        return const_cast<AccSet16 *>(this)->template at<RT, QT>();
    }
};

// Timing diagnostics only (results are wrong): build with -DNNS_DIAG -DNNS_FILTER_ABLATE=<bits>
//   1 no ring sync (wait + barrier), 2 no epilogue, 16 no DMA issue.  The product build (no NNS_DIAG)
// has none of the diagnostic switches: no ablation, no NNS_FILTER_CLOCK / NNS_DIAG_FILTER_ONLY
// environment variables (tests/test_abi_cpu.py greps the shipped library for them).
#if !defined(NNS_DIAG)
#undef NNS_FILTER_ABLATE
#undef NNS_F_NOLATCHFENCE
#undef NNS_F_NOLAG
#endif
#ifndef NNS_FILTER_ABLATE
#define NNS_FILTER_ABLATE 0
#endif
constexpr int kAblate = NNS_FILTER_ABLATE;

// ---- operand traits ---------------------------------------------------------------
// What every operator has unless it says otherwise.
struct OpBase {
    static constexpr bool kF16 = false;       // fp16 points (OpF16T): launched as filter_f16_kernel
    static constexpr bool kI8 = false;        // int8 points (OpI8): i32 accumulators, launched as filter_i8_kernel
    static constexpr bool kSplit = false;     // split-bf16 operands of fp32 points streamed hi, lo per k-step (OpSplitT)
    static constexpr bool kLazy = false;      // the lazy schedule of the split operands (OpLazySplitT)
    static constexpr bool kPre = false;       // the int8 pre-pass of the lazy schedule (OpI8Pre), launched as filter_i8pre_kernel
    static constexpr int kSlotSteps = 32;     // fragment steps (1 KiB each) of a ring slot
    static constexpr int kRingDepth = 4;      // ring slots
    static constexpr bool kDmaBurst = false;  // a slot's ring DMA pieces one per step (true: back to back, see the interval)
    static constexpr bool kTile16 = false;    // 32x32 MFMA tiles: a lane owns one query per query block
    static constexpr int kGroup = 1;          // intervals per workgroup barrier (OpI8Pre: NNS_F_PRE_GROUP, see pre_cadence_ok)
    static constexpr int kLPQ = 2;            // candidate lists (list lanes) per query and split: FilterGeom.lpq
    // the lanes' tau constants (c0, x2 per state) stay in registers: an LDS round trip on the slow path
    // queues behind the whole workgroup's fragment reads (measured: ~900 cycles each under this load)
    static constexpr bool kTauInRegs = true;
    using Acc = AccSet;
    // waves per workgroup: 8 = two per SIMD (<= 256 VGPRs each), 4 = one per SIMD (<= 512)
    static constexpr int kNW = 8;
    static constexpr int kPrefetch = 2;       // fragments in flight ahead of the MFMAs
};
// kQB = query blocks (of 32) per wave: their B operands stay resident in VGPRs (64 each at KT = 128).  More
// blocks = more MFMAs per LDS byte and per barrier interval, fewer waves' worth of registers.

// The ring of an operator: kRingDepth slots of kSlotSteps 1 KiB fragments + room for the slot's norms (up to 512 floats:
// the 16-deep tile; the lazy ring's slots never hold more than 256 refs)
template <class OP>
constexpr int F_D = OP::kRingDepth;
template <class OP>
constexpr int F_SLOT_COORD = OP::kSlotSteps * 1024;
template <class OP>
constexpr int F_SLOT_NORM = OP::kPre ? 256 : OP::kLazy ? 1024 : 2048;
template <class OP>
constexpr int F_SLOT_BYTES = F_SLOT_COORD<OP> + F_SLOT_NORM<OP>;
template <class OP>
constexpr int F_LDS_BYTES = F_D<OP> * F_SLOT_BYTES<OP>;

template <int SPB, int QB_>
struct OpF32T : OpBase {  // fp32 operands: float4 #b = operands of MFMA k-steps 4b .. 4b+3 (8 dims per fragment)
    static constexpr int kSPB = SPB;          // fragment steps per 32-point image block: KT = 8 * SPB
    // a slot's ring DMA pieces back to back (see the interval) — where it measured faster: KT = 128 (+0.65 % on long streams:
    // C3) and KT = 32 (+0.8 %); KT = 16 / 64 / 256 within -0.4 .. +0.1 %: one piece per step as before
    static constexpr bool kDmaBurst = SPB == 16 || SPB == 4;
    // SIMD partners half a block out of phase (+1.3 % on C3); a 2-step block (KT = 16) has no half to lag by
    static constexpr bool kLag = SPB >= 4;
    static constexpr int kQB = QB_;           // 4 * SPB resident operand registers per query block
    // (kPrefetch: 4 x 64 cycles per fragment)
    __device__ static __forceinline__ f32x16 mma(const float4 &a, const float4 &b, f32x16 acc)
    {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
        return acc;
    }
};
using OpF32 = OpF32T<16, 2>;      // KT = 128
using OpF32K32 = OpF32T<4, 2>;    // KT = 32: the mid-range dimensionalities (k = 17 .. 32)
// KT = 16: the reference driver's own 16-D samples (main.cu:38-51) without zero padding to 32: 2 fragment
// steps per 32-ref block, 16 blocks = 512 refs per ring slot (norms: two dwordx4 DMA pieces)
using OpF32K16 = OpF32T<2, 2>;
using OpF32K64 = OpF32T<8, 2>;    // KT = 64: 32 < k <= 64 without padding to 128
// KT = 256 (128 < k <= 256): the resident operands of ONE query block already take 128 registers,
// a ring slot holds one 32-ref block (32 KiB), and the ring turns twice as often per MFMA
using OpF32K256 = OpF32T<32, 1>;

// v_mfma_f32_32x32x16_bf16 on 16-byte fragments (8 bf16 = one operand): lane = query, 16 refs per lane — the C layout of
// the 32x32x2 f32 form.  The compiler builtin, not OpBF16T's in-place asm: with the 32x32 tile's two 16-register
// accumulators hipcc keeps every accumulator in one tuple (no extra copies against OpF32T, no scratch:
// tests/test_split_filter_cpu.py), and its hazard recognizer places the wait states in front of the epilogue's reads,
// which asm MFMAs would leave to hand-placed fences.
struct OpMma32x16 : OpBase {
    __device__ static __forceinline__ f32x16 mma(const float4 &a, const float4 &b, f32x16 acc)
    {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
    }
};

// Split-bf16 operands for fp32 points (the default for them; NNS_FILTER_F32 keeps OpF32T): every centred value v is
// h = rn_bf16(v) plus l = rn_bf16(v - h) (v - h is exact in fp32), and x'.y' is taken as the three products
// qh.rh + qh.rl + ql.rh on v_mfma_f32_32x32x16_bf16 (bf16 products are exact in fp32; the dropped terms are
// ~3 * 2^-16 sum |x'_t y'_t|: tau mode 3, nns_internal.h).  The K3 geometry unchanged: the 32x32x16 C layout is the
// 32x32x2 f32 one (a lane = one query column, 16 ref rows), and a 16-dim k-step is TWO 1 KiB fragments — hi, then
// lo — of 32 points x 16 dims x 2 B, so a block at each depth has the bytes, fragment steps and resident query
// registers of the fp32 block (KT = 8 * SPB).  Query fragment b of a block is qh (b even) / ql (b odd) of k-step
// b / 2; the MFMAs of ref fragment b: hi (b even) x qh, ql; lo (b odd) x qh — 3 MFMAs x 32 cycles per k-step and
// query block against 8 x 64 of OpF32T.
template <int SPB, int QB_>
struct OpSplitT : OpMma32x16 {
    static constexpr int kSPB = SPB;
    static constexpr bool kSplit = true;
    // (kDmaBurst: the bf16 operators' schedule — intervals ~5x shorter than OpF32T's)
    static constexpr bool kLag = SPB >= 4;    // (the lag of half a block keeps hi / lo pairs together: SPB / 2 is even)
    static constexpr int kQB = QB_;
    // (kPrefetch: 2 x 32 or 4 x 32 cycles per fragment)
};
using OpSplitK16 = OpSplitT<2, 2>;
using OpSplitK32 = OpSplitT<4, 2>;
using OpSplitK64 = OpSplitT<8, 2>;
using OpSplit = OpSplitT<16, 2>;   // KT = 128: C3
using OpSplitK256 = OpSplitT<32, 1>;

// bf16 points at KT = 128 / 256 / 512: v_mfma_f32_16x16x32_bf16.  Same flops per cycle as the 32x32x16 form,
// but the chip holds a ~14 % higher clock on it under this loop's load (measured here on C5:
// in-kernel clock 2.05 vs 1.80 GHz, filter 70 vs 80 ms in the bare loop; MI355X guide, 'DVFS
// give-back' item 7).  A step = one 1 KiB fragment (16 refs x 32 dims) x the wave's FOUR
// 16-query tiles; step b = 8 * rt + ks: the 8 k-steps of ref tile 0, then those of ref tile 1.
// C layout: lane l holds query column l & 15 and ref rows 4 * (l >> 4) .. + 3 of each tile, so a
// lane carries four queries (one per query tile) x 8 refs per block, and a query's refs are
// spread over the four lanes l & 15 + 16 g — four lane-private candidate lists per query.
//
// The record collection of one ref tile runs INSIDE the MFMA stream of the other: a burst of
// ~20 VALU instructions at a block boundary keeps the SIMD's vector issue port for ~80 cycles
// with no MFMA issued (neither by this wave nor by its SIMD partner: lagging the partners did
// not hide it, measured), which cost 7-9 % of this kernel.  Two v_min per MFMA gap fit the 8
// issue cycles a 16x16x32 leaves free, so the reduction of tile rt's finished scores is spread
// over k-step 1 of tile 1 - rt, and the threshold test + (rare) slow path follow at k-step 2.
//
// F16_: the same operator for fp16 points (OpF16T below) — v_mfma_f32_16x16x32_f16 has the bf16 form's rate, operand and
// result layout, so the mnemonic inside the two asm statements is the only difference.
template <int SPB_, int NW_ = 8, int QB_ = 2, bool F16_ = false>
struct OpBF16T : OpBase {
    static constexpr int kSPB = SPB_;         // 16: KT = 256 (8 k-steps per 16-ref tile); 8: KT = 128 (4 k-steps); 32: KT = 512
    static constexpr bool kTile16 = true;
    static constexpr int kLPQ = 4;            // every lane keeps the lists of its own rows
    static constexpr bool kLag = false;       // lock-step SIMD partners (lagging them: +1..4 % time on C5)
    static constexpr bool kTauInRegs = false; // 222-234 VGPRs: the four states' constants live in LDS (read on the slow path)
    using Acc = AccSet16;
    static constexpr int kQB = QB_;           // 2: 64 queries per wave = 4 query tiles; 1: 32 queries = 2 tiles
    static constexpr int kNW = NW_;
    // Inline asm, accumulating IN PLACE: through the builtin hipcc picks the three-address form
    // and rotates the eight 4-register accumulators through extra tuples (52-72 registers live
    // instead of 32), which spills the resident query operands.  The compiler does not see MFMA
    // hazards of an asm statement; the kernel keeps them by construction: an accumulator is
    // re-used as srcC only 8 MFMAs later, and VALU reads of it (the epilogue) wait behind
    // the epilogue's fences (mma16_tail_fence, the sched_barriers of t16_step).
    __device__ static __forceinline__ void mma16(const float4 &a, const float4 &b, f32x4 &acc)
    {
        if constexpr (F16_)
            asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0"
                         : "+v"(acc)
                         : "v"(__builtin_bit_cast(f32x4, a)), "v"(__builtin_bit_cast(f32x4, b)));
        else
            asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0"
                         : "+v"(acc)
                         : "v"(__builtin_bit_cast(f32x4, a)), "v"(__builtin_bit_cast(f32x4, b)));
    }
    // First MFMA of a tile: srcC = the refs' norms (three-address form).  The accumulator is an
    // in/out operand although its old value is not read: that pins every tile to ONE register
    // tuple for the whole kernel.  As a fresh output the allocator may give it another tuple and
    // reconcile at the loop back-edge with v_mov copies of the accumulators right behind the
    // interval's last MFMAs — a read hazard (caught by tools/check_mfma_hazards.py).
    __device__ static __forceinline__ void mma16_seed(const float4 &a, const float4 &b, f32x4 &acc, const f32x4 &c)
    {
        if constexpr (F16_)
            asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %3"
                         : "+v"(acc)
                         : "v"(__builtin_bit_cast(f32x4, a)), "v"(__builtin_bit_cast(f32x4, b)), "v"(c));
        else
            asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %3"
                         : "+v"(acc)
                         : "v"(__builtin_bit_cast(f32x4, a)), "v"(__builtin_bit_cast(f32x4, b)), "v"(c));
    }
    // VALU may read an accumulator 8 wait states after the MFMA that wrote it issued (what hipcc
    // inserts behind the builtin: s_nop 7).  To the compiler an asm MFMA's result is ready at
    // once.  In the loop the readers sit a whole step (>= 64 cycles) behind the writers and
    // __builtin_amdgcn_sched_barrier keeps them there; the kernel's tail reads right behind the
    // last MFMAs and needs the explicit wait, with the accumulators as in/out operands so that
    // the reads are ordered behind it.
    __device__ static __forceinline__ void mma16_tail_fence(AccSet16 &c)
    {
        if constexpr (QB_ == 1) asm volatile("s_nop 7" : "+v"(c.t10), "+v"(c.t11));   // (two query tiles per wave)
        else asm volatile("s_nop 7" : "+v"(c.t10), "+v"(c.t11), "+v"(c.t12), "+v"(c.t13));
    }
};
using OpBF16 = OpBF16T<16>;       // KT = 256
using OpBF16K128 = OpBF16T<8>;    // KT = 128: k <= 128 without padding to 256 (half the MFMAs)
// KT = 512: EIGHT waves x 32 queries (two query tiles per wave, 128 operand registers) = 256 queries per workgroup, two
// waves per SIMD — a partner issues MFMAs while a wave sits in an LDS-DMA issue.  A 1 KiB fragment feeds two MFMAs per
// wave: LDS fragment reads 32 of every 64 cycles.
using OpBF16K512T = OpBF16T<32, 8, 1>;
// fp16 points at KT = 256 / 128: OpBF16 / OpBF16K128 on v_mfma_f32_16x16x32_f16 (K2's order-1 image of binary16 operands,
// tau mode 4).  Ring, epilogue, lists and plan are the bf16 operators'.
template <int SPB_>
struct OpF16T : OpBF16T<SPB_, 8, 2, true> {
    static constexpr bool kF16 = true;
};
using OpF16 = OpF16T<16>;
using OpF16K128 = OpF16T<8>;

// int8 points at KT = 256: v_mfma_i32_16x16x64_i8.  A 1 KiB fragment is 16 points x 64 dims of bytes, so a 32-ref block is
// 2 ref tiles x 4 k-steps = 8 fragments — OpBF16K128's geometry byte for byte (8 KiB blocks, 4 per ring slot, four
// resident query fragments per 16-query tile: 64 operand registers), and ring, step schedule, record forms,
// thresholds, lists and slow path are that operator's.  What differs:
//   * the accumulators are i32, seeded with 0 (the inline constant as srcC), and hold x.y exactly: |x.y| <= 256 * 128^2 = 2^22;
//   * -2 v does not fit int8, so the image holds the values and the factor is applied where a tile RETIRES (t16_step,
//     k-step RET of the other tile; the stream's tail): retire() turns the tile's four accumulator registers IN PLACE into
//     the fp32 scores s = fma(-2, (float)acc, |y|^2) — v_cvt_f32_i32 + v_fma_f32 per element, both exact: (float)acc is an
//     integer of magnitude <= 2^22, the fp32 norm an integer <= 2^22, so |s| <= 2^22 + 2^23 < 2^24 is an integer fp32
//     holds, and the fma rounds nothing.  The norms are the registers the bf16 operator seeds its tiles with (nseed0 /
//     nseed1): tile rt's are loaded two steps before its first MFMA and stay until two steps before its next block's,
//     which is after its retirement.  Padding refs carry the norm +INF: fma(-2, x, +INF) = +INF, never recorded;
//   * everything behind the retirement (tile minimum, masks, threshold test, records) reads fp32 scores out of the same
//     registers as before, and the tile's next seed MFMA overwrites them without reading (srcC = 0).
// The MFMA is the compiler builtin: with 64 resident operand registers instead of OpBF16's 128 the allocator has room
// for the three-address form (no spills: tests/test_i8_cpu.py reads the ISA), and hipcc's hazard recognizer places the
// wait states between an MFMA and the VALU reads of its result, which the asm form leaves to hand-placed fences.
struct OpI8 : OpBF16T<8> {
    static constexpr bool kI8 = true;
    __device__ static __forceinline__ void mma16(const float4 &a, const float4 &b, f32x4 &acc)
    {
        acc = __builtin_bit_cast(f32x4, __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, a), __builtin_bit_cast(i32x4, b),
                                                                             __builtin_bit_cast(i32x4, acc), 0, 0, 0));
    }
    // first MFMA of a tile: srcC = 0 (the norms enter at the retirement)
    __device__ static __forceinline__ void mma16_seed(const float4 &a, const float4 &b, f32x4 &acc, const f32x4 &)
    {
        const i32x4 z = {0, 0, 0, 0};
        acc = __builtin_bit_cast(f32x4, __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, a), __builtin_bit_cast(i32x4, b), z, 0, 0, 0));
    }
    // (builtin MFMAs: the compiler keeps the read hazards)
    __device__ static __forceinline__ void mma16_tail_fence(AccSet16 &) {}
    // a finished tile's i32 dot products -> fp32 scores |y|^2 - 2 x.y, in place (exact: see above)
    __device__ static __forceinline__ void retire(f32x4 &acc, const f32x4 &norm)
    {
        const i32x4 d = __builtin_bit_cast(i32x4, acc);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(-2.0f, (float)d[e], norm[e]);
    }
};

// The deep bf16 tiles whose blocks do not divide a ring slot (KT 384, 640, 768, 1024) run v_mfma_f32_32x32x16_bf16 with
// ONE query block per wave.
template <int SPB_, int QB_, int NW_ = 8, bool LAG_ = (NW_ == 8)>
struct OpBF16T32T : OpMma32x16 {
    static constexpr int kSPB = SPB_;         // fragment steps (16 dims each) per 32-ref block
    static constexpr bool kLag = LAG_;        // (one wave per SIMD has no partner to stagger against)
    static constexpr int kQB = QB_;
    static constexpr int kNW = NW_;
    // (kPrefetch: one MFMA (32 cycles) per fragment and query block)
};
// KT = 1024 (512 < k <= 1024): K-split accumulation.  The resident operands of one query block are 256
// registers, so a workgroup is FOUR waves (one per SIMD, up to 512 registers each) = 128 queries; a 32-ref
// block is 64 fragment steps = TWO ring slots, and its accumulators carry across the slot barrier: seeded at
// step 0 of the even slot, retired at step 31 of the odd one.  One MFMA per 1 KiB LDS fragment:
// LDS-bandwidth bound (~50 % of the bf16 MFMA peak), still ~50x the exact VALU scan.
using OpBF16K1024 = OpBF16T32T<64, 1, 4>;
// KT = 768 (512 < k <= 768): 48 fragment steps per block — two blocks over three ring slots.  The resident
// operands of one query block are 192 registers, so — unlike at 1024 — TWO waves per SIMD fit (<= 256 registers
// each): eight waves = 256 queries per workgroup, and a SIMD partner covers a wave's LDS-DMA issue stalls (the
// one-wave-per-SIMD tiles lose about half their MFMA slots to them: profiles/r03_deep_ablate.txt).  Lock-step
// partners (a half-block lag would straddle slots).
using OpBF16K768 = OpBF16T32T<48, 1, 8, false>;
// KT = 640 (512 < k <= 640): 40 fragment steps per block — FOUR blocks over FIVE ring slots; 160 operand registers, eight waves
using OpBF16K640 = OpBF16T32T<40, 1, 8, false>;
// KT = 384 (256 < k <= 384): the same form below 512 — 24 steps per block, four blocks over three slots, 96 operand
// registers; k = 300 ran on the 512-deep tile at 36 % of peak
using OpBF16K384 = OpBF16T32T<24, 1, 8, false>;

// Lazy split ("lazy split"): the split operands in a schedule that runs the two cross products only where the result
// needs them.  The kernel uses a score to ask "is the minimum of this 32 x 32 tile within the lane's threshold?"; the
// cross products qh.rl + ql.rh move a score by at most B (split_lazy_bound, nns_internal.h: ~2^-6 |x'||y'|), so a tile
// whose hi-hi scores all lie above thr + B is retired after ONE product per k-step.  A flagged tile (wave-uniform, the
// slow path of the eager form plus a few per cent of the tiles early in a stream) continues the SAME accumulator with
// the 2 * KT / 16 cross MFMAs — rh re-read from the ring slot, rl loaded straight from the lo region of K2's lazy image
// — and then runs record_all on the three-product scores as the eager kernel does.  Only the hi fragments stream
// through LDS: a 64-ref slot is kSlotSteps = 16 fragment steps (16 KiB), and the LDS the lo halves no longer take makes
// the ring eight slots deep (an interval is a third of the eager one, the DMA latency is not).
// kSPB = HI fragments per block (KT / 16); the resident query operands are the eager ones (qh, ql per k-step).
template <int SPB, int QB_>
struct OpLazySplitT : OpMma32x16 {
    static constexpr int kSPB = SPB;
    static constexpr int kSlotSteps = 16;
    static constexpr int kRingDepth = 8;
    static constexpr bool kLazy = true;       // (kSplit stays false: that is the eager stream of hi AND lo fragments)
    static constexpr bool kLag = SPB >= 4;
    static constexpr int kQB = QB_;
};
using OpLazySplit = OpLazySplitT<8, 2>;   // KT = 128: C3

// The lazy schedule on v_mfma_f32_16x16x32_bf16 (KT = 128): OpBF16K128's step (t16_step: in-place asm MFMAs, the
// retiring tile's minima behind the other tile's MFMAs, one cold branch) over OpLazySplitT's ring (16-step slots of hi
// fragments, eight deep), reading the SAME image — K2 form 3, whose fragments are in the 32x32x16 operand order — with a
// per-lane gather (lazy16_gather, nns_internal.h): a 16x16x32 operand of ref tile t, k-step ks is 16 bytes per lane out
// of the two adjacent 1 KiB fragments 2 ks, 2 ks + 1, every byte of the slot still read once per wave, and each
// ds_read_b128 lane group covers one 256-byte bank row exactly once.  The masks compare the hi-hi minima against
// fl(thr + B); a flagged (ref tile, state) gets its cross products on 16x16x32 too (t16_refine).  A query sits on four
// lanes g = 0 .. 3; the lists stay two per query (kLPQ = 2: the plan, the list format and K5 are OpLazySplit's), owned by
// the lanes with even g, to which lane g ^ 1 hands its refined scores through a row swap.
struct OpLazySplit16 : OpBF16T<8> {
    static constexpr int kSlotSteps = 16;
    static constexpr int kRingDepth = 8;
    static constexpr bool kLazy = true;
    static constexpr int kLPQ = 2;
};

// The int8 pre-pass of the lazy schedule (KT = 128; DESIGN section 4, "int8 pre-pass"): the first-pass question — can any
// pair of this 16 x 16 tile be within the lane's threshold? — asked of v_mfma_i32_16x16x64_i8 on K2's int8 image of the
// same centred points (r8, q8 under one scale s; the image holds -r8 and the accumulator is seeded with N_j =
// floor(|y'_j|^2 / (2 s^2)), so it ends as A = N_j - q8.r8 with 2 s^2 A <= score + B8_i).  Half the MFMA cycles and half
// the ring bytes of the hi-hi pass: a 32-ref block is 2 ref tiles x 2 k-steps of 64 dims = 4 fragments, a 64-ref slot 8
// fragment steps (one DMA piece per wave) + the slot's 64 seeds, and the ring is 16 slots deep so that a piece keeps its
// landing time at half the interval.  The threshold lives in the integer domain (thrw8, updated where thr is): the
// hot loop spends v_min3_i32 + v_min_i32 + v_cmp per (tile, state).  A tile has only two k-steps, so the retiring tile's
// minima and masks are taken at k-step 1 of the other tile and tested one step later, at its own seed step; a flagged
// (tile, state) is refined on a FRESH accumulator with lazy16's chain in lazy16's order (norms, four rh.qh, then rh.ql and
// rl.qh per k-step), every operand loaded from global memory inside the branch.  Lists, plan and K5 are OpLazySplit16's.
struct OpI8Pre : OpBF16T<4> {
    static constexpr int kSlotSteps = 8;
    static constexpr int kRingDepth = kI8PreRingDepth;
    static constexpr bool kPre = true;
    // One barrier per kGroup intervals.  A refinement stalls its wave for longer than an interval; with a barrier at every
    // interval the seven other waves wait it out, with one per group they run on inside the group and the stalled wave's
    // SIMD partner has the MFMA pipe to itself meanwhile.  A wave's thresholds depend on its own stream alone, so the lists
    // are the same whatever the cadence.
    static constexpr int kGroup = kI8PreGroup;
    static constexpr int kLPQ = 2;
    // (the builtin, as OpI8: 32 resident operand registers leave the allocator room, and it keeps the read hazards)
    __device__ static __forceinline__ void mma16(const float4 &a, const float4 &b, f32x4 &acc)
    {
        acc = __builtin_bit_cast(f32x4, __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, a), __builtin_bit_cast(i32x4, b),
                                                                             __builtin_bit_cast(i32x4, acc), 0, 0, 0));
    }
    // first MFMA of a tile: srcC = the refs' integer seeds
    __device__ static __forceinline__ void mma16_seed(const float4 &a, const float4 &b, f32x4 &acc, const f32x4 &c)
    {
        acc = __builtin_bit_cast(f32x4, __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, a), __builtin_bit_cast(i32x4, b),
                                                                             __builtin_bit_cast(i32x4, c), 0, 0, 0));
    }
    __device__ static __forceinline__ void mma16_tail_fence(AccSet16 &) {}
    // the refinement's bf16 MFMAs (builtin too)
    __device__ static __forceinline__ f32x4 mma16_bf16(const float4 &a, const float4 &b, const f32x4 &acc)
    {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
    }
};

// min over the lanes that carry the same query: l ^ 32 (32x32 tiles), and l ^ 16 too (16x16 tiles).  Row
// swaps (v_permlane32_swap / v_permlane16_swap, gfx950), not ds_bpermute: no LDS round trip on the slow
// path.  swap(t, t) returns {old t with its upper rows replaced by the partner's, and vice versa}: the min of
// the two halves of the pair is min(t[l], t[l ^ 32]) on every lane (checked on hardware:
// nns_selftest_lane_share).
template <bool T16>
__device__ __forceinline__ float share_min(float t)
{
    const unsigned tb = __float_as_uint(t);
    const auto s32 = __builtin_amdgcn_permlane32_swap(tb, tb, false, false);
    t = fminf(__uint_as_float(s32[0]), __uint_as_float(s32[1]));          // min(t[l], t[l ^ 32])
    if constexpr (T16) {
        const unsigned tb2 = __float_as_uint(t);
        const auto s16 = __builtin_amdgcn_permlane16_swap(tb2, tb2, false, false);
        t = fminf(__uint_as_float(s16[0]), __uint_as_float(s16[1]));      // min(t[l], t[l ^ 16])
    }
    return t;
}

struct FilterArgs {
    const float4 *qimg;     // [m_pad/32][16][64] 16-byte fragments
    const char *rimg;       // [n_pad/32][16 KiB]
    const char *rimg_lo;    // lazy image layout (K2 form 3): rimg holds the blocks' hi fragments back to back, rimg_lo the lo
                            // fragments with the same block indexing; nullptr: the eager layout (hi, lo interleaved per k-step)
    const float *rnorm;     // [n_pad]
    const float *qnorm;     // [m_pad]
    const DevScalars *scal;
    CandEntry *lists;       // [splits][m_pad/32][kCandCap][64 lanes]
    int *counts;            // [splits][m_pad/32][64 lanes]
    int total_slots, slots_per_split, m_pad, kt;
    int tau_mode;           // TAU_F32 .. TAU_F16 (filter_tau_mode)
    int share_thr;          // short streams: a query's lanes adopt the smallest of their thresholds
    int tile_rec;           // short streams: ONE record per (lane, ref tile) — (tile minimum, first ref of the lane's
                            // rows) — instead of one per score within the threshold; K5 re-ranks the lane's rows
    FilterPreArgs pre;      // OpI8Pre: K2's int8 operands beside the lazy image
#ifdef NNS_DIAG
    unsigned long long *stamps;   // diagnostic (NNS_FILTER_CLOCK): per-workgroup s_memtime / s_memrealtime
#endif
};

template <class OP>
__device__ __forceinline__ void filter_main(const FilterArgs &a)
{
    constexpr int F_NW = OP::kNW;
    constexpr int SPB = OP::kSPB;                      // fragment steps per image block
    // Blocks and ring slots (ring_geom, nns_internal.h): up to a slot's steps per block a slot holds BPS whole blocks;
    // deeper blocks straddle slots with a SUPER-PERIOD of SUP_SLOTS slots = SUP_BLKS blocks, e.g. 48 steps (768-deep):
    // 3 slots = 2 blocks, the second one starting in the middle of the second slot.  Accumulators carry across the slot
    // barriers; every slot of a super-period brings the norms of all its blocks.
    // The lazy split operator streams hi fragments only: its slots are SPS = 16 steps in a ring of 8 (see OpLazySplitT);
    // everywhere else SPS = 32, F_D = 4.
    constexpr bool LAZY = OP::kLazy;
    constexpr int SPS = OP::kSlotSteps;
    static_assert(F_LDS_BYTES<OP> == 4 * (32768 + 2048) || (OP::kPre && F_LDS_BYTES<OP> <= 4 * (32768 + 2048)),
                  "every operator's ring takes the same LDS: one workgroup per CU");
    constexpr RingGeom RG = ring_geom(SPB, SPS);
    constexpr bool DEEP = RG.deep;
    static_assert(SPS == 32 || !DEEP, "blocks straddling slots: 32-step slots only");
    constexpr int SUP_SLOTS = RG.slots;
    constexpr int SUP_BLKS = RG.blocks;
    constexpr int SPBLK = SUP_SLOTS;                   // (name kept: slots of a deep block's super-period)
    constexpr int BPS = DEEP ? 1 : SPS / SPB;          // image blocks per ring slot (shallow tiles)
    constexpr int BLK_BYTES = SPB * 1024;
    constexpr int SLOT_REFS = RG.slot_refs;          // norms DMAed with a slot
    constexpr int F_PPW = F_SLOT_COORD<OP> / 1024 / F_NW;   // 1 KiB DMA pieces per wave per slot
    static_assert((SPS % SPB == 0 && SPB >= 2) || SPB == 64 || SPB == 48 || SPB == 40 || SPB == 24, "a slot is SPS fragment steps");
    static_assert(SUP_SLOTS * SPS == SUP_BLKS * SPB, "a super-period is whole slots and whole blocks");
    static_assert(SPBLK == 1 || (!OP::kLag && !OP::kTile16), "blocks straddling slots: lock-step 32x32 tiles only");
    static_assert(SLOT_REFS == 32 || SLOT_REFS == 64 || SLOT_REFS == 128 || SLOT_REFS == 256 || SLOT_REFS == 512,
                  "norm pieces: one dword per lane, or dwordx4 pieces of 256 norms");
    constexpr int F_NP = SLOT_REFS <= 256 ? 1 : SLOT_REFS / 256;   // norm DMA pieces per slot
    static_assert(SLOT_REFS * 4 <= F_SLOT_NORM<OP>, "norm room of a ring slot");
    // How far ahead of its interval a slot's DMA is issued.  Lagging SIMD partners still read slot s - 1 during
    // the first half of interval s, so with four ring slots they can fill slot s + 2 at most: ONE interval between
    // issue and deadline — plenty when an interval is 16 000 cycles (fp32 tiles), not when it is 1 000 - 4 000
    // (bf16 tiles: a 1 KiB piece takes ~2 600 cycles from issue to landed under load, and round 2's waves sat in
    // vmcnt(0) for half their cycles at the deep tiles).  Lock-step operators are done with slot s - 1 at the
    // barrier that opens interval s, so they fill slot s + 3 = s - 1 (mod 4) and wait with a COUNTED vmcnt that
    // leaves the youngest slot's pieces in flight across the barrier: TWO intervals of latency cover.
    // The lazy ring of eight: lagging partners may fill slot s + 6 at most; NNS_F_LAZY_AHEAD slots ahead (A/B builds: 2 .. 6).
#ifndef NNS_F_LAZY_AHEAD
#define NNS_F_LAZY_AHEAD 4
#endif
    // A query's two lanes adopt the smaller of their thresholds in the lazy kernel whatever the stream length (tighten);
    // 0: only where the plan says so (A/B builds)
#ifndef NNS_F_LAZY_SHARE
#define NNS_F_LAZY_SHARE 1
#endif
    constexpr bool kLazyShare = NNS_F_LAZY_SHARE != 0;
    // The pre-pass ring of sixteen: an interval is half the lazy one, so twice as many slots ahead keep a piece's landing time
    // (NNS_F_PRE_AHEAD, default 8: nns_internal.h)
    constexpr bool PRE = OP::kPre;
    constexpr int AHEAD = PRE ? kI8PreAhead : LAZY ? NNS_F_LAZY_AHEAD : OP::kLag ? 2 : 3;
    static_assert(AHEAD >= 2 && AHEAD <= F_D<OP> - (OP::kLag ? 2 : 1), "a slot is refilled only when no wave reads it any more");
    // Barrier cadence: sync_slot runs at the intervals s with s % G == 0 and confirms the G slots after slot s
    constexpr int G = OP::kGroup;
    static_assert(G == 1 || PRE, "a barrier at every interval everywhere but in the pre-pass");
    static_assert(!PRE || pre_cadence_ok(F_D<OP>, AHEAD, G), "pre-pass ring: G < AHEAD and AHEAD + G <= ring depth");
    // DMA pieces per wave and slot that the counted vmcnt waits may leave in flight: with the norms issued by one wave
    // per slot, a wave's youngest slot has F_PPW or F_PPW + F_NP pieces — counting F_PPW is safe for both
    // (not the 768-deep tile: 252 of its 256 registers are taken, the turn-taking test spills)
    constexpr bool NORM_ONE = SPB != 48;
    constexpr int F_PPS = NORM_ONE ? F_PPW : F_PPW + F_NP;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5;
    constexpr int QB = OP::kQB;
    static_assert(QB <= 2, "the accumulator sets hold two query blocks");
    const int qblk0 = (blockIdx.x * F_NW + wave) * QB;
    // Lane STATES: the running minimum / threshold / candidate list a lane keeps per query it
    // carries.  32x32 tiles: one query per query block (state = block, 16 scores per ref block);
    // 16x16 tiles: one query per 16-query tile (state = tile, 8 scores per ref block).
    constexpr bool T16 = OP::kTile16;
    constexpr int NS = T16 ? 2 * QB : QB;
    constexpr int QPS = T16 ? 16 : 32;          // queries per state
    // query fragments per 32-query block of the fp32 points' image (lazy: qh and ql of each hi step; the pre-pass refines
    // out of the same image: 16 at KT = 128)
    constexpr int QFB = PRE ? 16 : LAZY ? 2 * SPB : SPB;
    constexpr int NBQ = T16 ? SPB / 2 : QFB;    // resident operand fragments per state (the pre-pass: q8's two k-steps)
    // the lazy schedule on 16x16 tiles (OpLazySplit16): gathered operands, two lists per query
    constexpr bool L16 = LAZY && T16;
    static_assert(!L16 || (OP::kLPQ == 2 && QB == 2 && SPB == 8), "OpLazySplit16: KT = 128, four states, two lists per query");
    // the pre-pass keeps OpLazySplit16's lists: two per query, owned by the lanes with even g
    constexpr bool Q2 = L16 || PRE;
    static_assert(!PRE || (T16 && !LAZY && OP::kLPQ == 2 && QB == 2 && SPB == 4), "OpI8Pre: KT = 128, four states, two lists per query");
    static_assert(Q2 || OP::kLPQ == (T16 ? 4 : 2), "list lanes per query: the lanes a query sits on");
    const int g16 = lane >> 4, i16 = lane & 15;   // (16x16 tiles: the lane's row quarter and query column)

    // ---- resident B operands: this wave's QB x 32 queries, all of K (128 VGPRs at QB = 2) ----
    float4 bq[NS][NBQ];
    TauConsts tc[NS];
    float bnd[NS];   // lazy split: B, how far a pair's three-product score can lie below its hi-hi score
#pragma unroll
    for (int st = 0; st < NS; ++st) bnd[st] = 0.0f;
    {
        const float4 *src = a.qimg + (size_t)qblk0 * (QFB * 64) + lane;
#pragma unroll
        for (int st = 0; st < NS; ++st) {
#pragma unroll
            for (int b = 0; b < NBQ; ++b) {
                // (L16: qh of query tile st, k-step b, gathered out of query block st / 2's interleaved qh | ql fragments)
                if constexpr (L16) bq[st][b] = a.qimg[(size_t)(qblk0 + (st >> 1)) * (QFB * 64) + lazy16_gather(lane, st & 1, b, 2, 0)];
                else if constexpr (PRE) bq[st][b] = a.pre.q8[((size_t)(qblk0 * 2 + st) * 2 + b) * 64 + lane];   // q8 of query tile st, k-step b
                else bq[st][b] = src[(st * NBQ + b) * 64];
            }
            // (record form 2 keeps no thresholds: skip the margin's double-precision arithmetic, ~1 us of a short stream)
            if (T16 || a.tile_rec != 2)
                tc[st] = tau_consts(a.kt, a.qnorm[qblk0 * 32 + st * QPS + (lane & (QPS - 1))],
                                    __uint_as_float(a.scal->ymax2_bits), a.tau_mode);
            else
                tc[st] = TauConsts{0.0f, 0.0f, 0.0f};
            if constexpr (LAZY)
                bnd[st] = split_lazy_bound(a.kt, a.qnorm[qblk0 * 32 + st * QPS + (lane & (QPS - 1))],
                                           __uint_as_float(a.scal->ymax2_bits));
            if constexpr (PRE) bnd[st] = a.pre.qb8[qblk0 * 32 + st * QPS + (lane & (QPS - 1))];   // B8 of the lane's query
        }
    }
    // (pre-pass) score units per integer unit: 1 / (2 s^2), s = cmax / 127 as K2 forms it
    float inv2s2 = 0.0f;
    if constexpr (PRE) {
        const float s8 = __uint_as_float(a.scal->i8_cmax_bits) / 127.0f;
        inv2s2 = 1.0f / (2.0f * s8 * s8);
    }
    // Pin the loads here: hipcc must wait for them BEFORE the ring starts, not with a
    // vmcnt(0) at their first use inside the loop (it cannot see the asm DMAs).
#pragma unroll
    for (int st = 0; st < NS; ++st) {
#pragma unroll
        for (int b = 0; b < NBQ; ++b)
            asm volatile("" : "+v"(bq[st][b].x), "+v"(bq[st][b].y), "+v"(bq[st][b].z), "+v"(bq[st][b].w));
        asm volatile("" : "+v"(tc[st].c0), "+v"(tc[st].c1), "+v"(tc[st].x2));
        if constexpr (LAZY || PRE) asm volatile("" : "+v"(bnd[st]));
    }
    // The tau constants of the lane's states live in LDS behind the ring (2 KiB per wave, read only on
    // the slow path) instead of 3 registers per state; c1 depends on the tile depth alone and is
    // wave-uniform
    float *tcl = reinterpret_cast<float *>(smem + F_LDS_BYTES<OP>) + wave * 512 + lane;
    if constexpr (!OP::kTauInRegs) {
#pragma unroll
        for (int st = 0; st < NS; ++st) {
            tcl[(2 * st) * 64] = tc[st].c0;
            tcl[(2 * st + 1) * 64] = tc[st].x2;
        }
    }
    const float c1u = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(tc[0].c1)));

#ifdef NNS_DIAG
    unsigned long long st_t0 = 0, st_r0 = 0;
    if (a.stamps) {   // diagnostic launches only: in-kernel clock = d(memtime) / d(memrealtime) * 100 MHz
        st_t0 = __builtin_amdgcn_s_memtime();
        st_r0 = __builtin_amdgcn_s_memrealtime();
    }
#endif
    const int slot0 = blockIdx.y * a.slots_per_split;
    int ns = a.total_slots - slot0;
    if (ns > a.slots_per_split) ns = a.slots_per_split;
    const unsigned lds_base = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)smem);

    // DMA piece p (0 .. F_PPW-1: 1 KiB image pieces; F_PPW .. F_PPW+F_NP-1: the norms) of slot s
    // (relative to slot0) into ring position s % F_D
    auto issue_piece = [&](int s, int p) __attribute__((always_inline)) {
        const size_t gslot = (size_t)(slot0 + s);
        const unsigned dst = lds_base + (s & (F_D<OP> - 1)) * F_SLOT_BYTES<OP>;
        if constexpr (PRE) {
            // the int8 region's slot (one 1 KiB piece per wave), and the slot's 64 seeds (one wave's business, as the norms)
            if (p < F_PPW) dma16(a.pre.rimg8 + gslot * F_SLOT_COORD<OP> + wave * 1024 + lane * 16, dst + wave * 1024);
            else if (((int)gslot & (F_NW - 1)) == wave) dma4(a.pre.rseed + gslot * SLOT_REFS + lane, dst + F_SLOT_COORD<OP>);
            return;
        }
        if (p < F_PPW) {
            const int piece = wave * F_PPW + p;
            if constexpr (OP::kSplit) {
                if (a.rimg_lo) {
                    // an eager kernel on the lazy image (the short-stream record forms of an index whose long streams run
                    // the lazy kernel): LDS fragment `piece` = block piece / SPB, k-step (piece % SPB) / 2, hi (even) or lo
                    const int pb = piece / SPB, pf = piece % SPB;
                    const char *reg = (pf & 1) ? a.rimg_lo : a.rimg;
                    dma16(reg + ((gslot * BPS + pb) * (SPB / 2) + (pf >> 1)) * 1024 + lane * 16, dst + piece * 1024);
                    return;
                }
            }
            dma16(a.rimg + gslot * F_SLOT_COORD<OP> + piece * 1024 + lane * 16, dst + piece * 1024);
        } else if (NORM_ONE && ((int)gslot & (F_NW - 1)) != wave) {
            // the slot's norms are ONE wave's business, the waves taking turns slot by slot (round 1 - 3: every wave copied
            // the same bytes to the same words, to keep the DMA counts per slot identical — eight pieces where one does,
            // and an LDS-DMA piece costs its SIMD ~130 cycles of MFMA issue whatever its size); the counted vmcnt waits
            // below therefore count IMAGE pieces only (a wave whose youngest slot carries norm pieces waits for them too)
        } else if constexpr (SLOT_REFS <= 64) {   // (128- and 256-ref slots: one dwordx4 piece of 256 norms)
            // (a 32-ref slot also copies the next slot's 32)
            dma4(a.rnorm + (gslot / SPBLK) * SLOT_REFS + lane, dst + F_SLOT_COORD<OP>);   // (a deep block: both its slots)
        } else {
            const int np = p - F_PPW;             // 256 norms per piece (a deep block: its super-period's, + over-read)
            dma16(a.rnorm + (gslot / SPBLK) * SLOT_REFS + np * 256 + lane * 4, dst + F_SLOT_COORD<OP> + np * 1024);
        }
    };
    auto issue = [&](int s) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < F_PPW + F_NP; ++p) issue_piece(s, p);
    };

    // ---- per-lane record state ---------------------------------------------------------
    float thr[NS];
    float thrw[NS];   // lazy split: fl(thr + B), what a tile's hi-hi minimum is tested against
    int thrw8[NS];    // pre-pass: (thr + B8) / (2 s^2) rounded up, what a tile's integer minimum is tested against
    int cnt[NS];
    // candidate lists are stored [split][state unit][entry][lane] (unit = the 64 lanes' lists of
    // one query block / query tile) so that both the appends of a wave and K5's per-query reads
    // touch consecutive 8-byte words
    // (L16: units of 32 queries as on 32x32 tiles; the owner of state st, quarter g, query i — g even — keeps list lane
    //  32 (g >> 1) + 16 (st & 1) + i of unit st >> 1)
    constexpr int LQPS = Q2 ? 32 : QPS;
    const size_t lblk0 = (size_t)blockIdx.y * (a.m_pad / LQPS) + (size_t)qblk0 * (32 / LQPS);
    const bool owner = !Q2 || (g16 & 1) == 0;
#pragma unroll
    for (int st = 0; st < NS; ++st) {
        thr[st] = thrw[st] = __builtin_inff();
        thrw8[st] = kI8PreThrMax;
#if defined(NNS_DIAG) && defined(NNS_F_THR_NEGINF)   // timing experiment: the fast path alone (results are wrong)
        thr[st] = thrw[st] = -__builtin_inff();
        thrw8[st] = -kI8PreThrMax;
#endif
        cnt[st] = 0;
    }
    // The same lists as a wave-uniform base (SGPR pair) + a 32-bit per-lane byte offset: the appends of the
    // slow path then need no 64-bit VALU address arithmetic (global_store saddr + voffset)
    char *lbase;
    {
        const uintptr_t lb = (uintptr_t)(a.lists + lblk0 * (kCandCap * 64));
        // (readfirstlane returns a signed int: go through unsigned, or a low word with bit 31 set
        //  sign-extends over the high half)
        const unsigned lb_hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(lb >> 32));
        const unsigned lb_lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)lb);
        lbase = (char *)(((uintptr_t)lb_hi << 32) | (uintptr_t)lb_lo);
    }
    const unsigned loff = (Q2 ? 32 * (g16 >> 1) + i16 : lane) * (unsigned)sizeof(CandEntry);
    // byte offset of state st's list behind lbase + loff
    auto list_off = [](int st) __attribute__((always_inline)) -> unsigned {
        if constexpr (Q2) return (unsigned)((st >> 1) * (kCandCap * 64) + (st & 1) * 16) * (unsigned)sizeof(CandEntry);
        else return (unsigned)(st * (kCandCap * 64 * (int)sizeof(CandEntry)));
    };
    f32x4 nseed0 = {0.0f, 0.0f, 0.0f, 0.0f}, nseed1 = nseed0;   // 16x16 tiles: the two ref tiles' norms
    // (OpI8: the stream's first retirement is of the start accumulators — 0 under the norm +INF: score +INF, nothing to record)
    if constexpr (OP::kI8) nseed1 = f32x4{__builtin_inff(), __builtin_inff(), __builtin_inff(), __builtin_inff()};
    // accumulators start at |y'_j|^2 of their rows: rows (r&3) + 8(r>>2) + 4h
    auto seed = [&](typename OP::Acc &acc, const char *slot, int blk) __attribute__((always_inline)) {
        if constexpr (T16) {
            return;   // (16x16 tiles: seed16 below)
        } else {
        const float *nrm = reinterpret_cast<const float *>(slot + F_SLOT_COORD<OP>) + blk * 32 + 4 * h;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 nv = *reinterpret_cast<const float4 *>(nrm + 8 * g);
            // (compile-time qb: a runtime-looking index would send the accumulators to scratch)
            static_for<QB>([&](auto qc) __attribute__((always_inline)) {
                constexpr int qb = decltype(qc)::value;
                acc.template at<qb>()[4 * g + 0] = nv.x;
                acc.template at<qb>()[4 * g + 1] = nv.y;
                acc.template at<qb>()[4 * g + 2] = nv.z;
                acc.template at<qb>()[4 * g + 3] = nv.w;
            });
        }
        }
    };
    // Shallow lock-step tiles (KT = 16: a tile is two steps, and both SIMD partners reach their tile boundaries
    // together): the NEXT tile's norms are read a whole tile ahead into 16 registers, so the tile's first MFMA does not
    // wait for an LDS round trip every 8 MFMAs (at the deeper tiles the lagging partner's MFMA chain covers it).
    constexpr bool kSeedAhead = !T16 && !OP::kLag && SPB <= 4;
    float4 nsd[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) nsd[g] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    auto seed_fetch = [&](const char *slot, int blk) __attribute__((always_inline)) {
        if constexpr (kSeedAhead) {
            const float *nrm = reinterpret_cast<const float *>(slot + F_SLOT_COORD<OP>) + blk * 32 + 4 * h;
#pragma unroll
            for (int g = 0; g < 4; ++g) nsd[g] = *reinterpret_cast<const float4 *>(nrm + 8 * g);
        }
    };
    auto seed_apply = [&](typename OP::Acc &acc) __attribute__((always_inline)) {
        if constexpr (kSeedAhead) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                static_for<QB>([&](auto qc) __attribute__((always_inline)) {
                    constexpr int qb = decltype(qc)::value;
                    acc.template at<qb>()[4 * g + 0] = nsd[g].x;
                    acc.template at<qb>()[4 * g + 1] = nsd[g].y;
                    acc.template at<qb>()[4 * g + 2] = nsd[g].z;
                    acc.template at<qb>()[4 * g + 3] = nsd[g].w;
                });
            }
        }
    };
    // 16x16 tiles: the norms of ref tile rt of block blk (rows 16 rt + 4 (lane >> 4) + i), loaded
    // two steps ahead of the tile's first MFMAs, which take them as srcC (no register copies)
    auto seed16 = [&](const char *slot, int blk, auto rt_c) __attribute__((always_inline)) {
        constexpr int rt = decltype(rt_c)::value;
        const float4 nv = *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(slot + F_SLOT_COORD<OP>) +
                                                            blk * 32 + 16 * rt + 4 * (lane >> 4));
        if constexpr (rt == 0) nseed0 = f32x4{nv.x, nv.y, nv.z, nv.w};
        else nseed1 = f32x4{nv.x, nv.y, nv.z, nv.w};
    };
    // one finished score x of ref j (slow path): append to the state's candidate ring, tighten
    // Slow path, step 1: tighten the lane's threshold with the minimum tmin of the scores about to be
    // examined.  Doing this FIRST is what keeps the slow path short: every ref within tau of the
    // FINAL minimum is below every threshold the lane ever holds (thresholds only shrink), so
    // appending against the already-tightened threshold still collects all of them, while a run of
    // descending scores no longer appends (and stores) each one.
    auto tighten = [&](auto st_c, float tmin) __attribute__((always_inline)) {
        constexpr int st = decltype(st_c)::value;
        // x -> x + 1.002 tau(x) is monotone, so the threshold of the running minimum is the minimum
        // of the thresholds: no separate running-minimum register.  (1.002: a hair wider than K5's
        // own tau, so that the lists are supersets of what K5 needs.)
        float c0v, x2v;
        if constexpr (OP::kTauInRegs) {
            c0v = tc[st].c0;
            x2v = tc[st].x2;
        } else {
            c0v = tcl[(2 * st) * 64];
            x2v = tcl[(2 * st + 1) * 64];
        }
        const float d = tmin + x2v;
        const float tn = tmin + (c0v + c1u * (d > 0.0f ? d : 0.0f)) * 1.002f;
        float t = tn < thr[st] ? tn : thr[st];
        // A query lives on 2 (32x32 tiles: lanes l, l ^ 32) or 4 (16x16: l ^ 16, l ^ 32) lanes, each seeing
        // a different part of every ref block.  Any of their thresholds is valid for all of them (each
        // is >= final minimum + tau), so they may adopt the smallest: a lane then stops taking the slow
        // path for refs a sibling lane has already beaten.  Pays on SHORT ref streams (where nearly
        // every tile is slow), costs 0.2 % on C3 / C5: a launch-time choice by stream length
        // (launch_filter).  Row swaps (v_permlane32_swap / 16_swap, gfx950), not ds_bpermute: no LDS
        // round trip.  (Wave-uniform slow path: every lane is active here.)
        // The LAZY kernel shares on long streams too (NNS_F_LAZY_SHARE, in the kernel: the plan's share_thr stays what
        // it is).  There a flag costs a refinement — 8 global loads, a wait that also drains the wave's ring pieces, and
        // 16 MFMAs: ~1900 cycles of the wave, ~185 of the workgroup — not the eager kernel's few dozen VALU
        // instructions, and one record process over a query's n refs flags 43 % fewer tiles than two private ones over
        // n / 2 each (C3: 3.40 % -> 1.93 % of the retirements, filter 13.70 -> 13.05 ms; DESIGN, "Where the lazy
        // kernel's time goes").  Lists only get shorter; every entry K5 needs is still <= every threshold the lane holds.
        // (the pre-pass always: its two lists per query rely on the four lanes holding one threshold)
        if (a.share_thr || (LAZY && kLazyShare) || PRE) t = share_min<T16>(t);
        // (a finite threshold: "x <= thr" then also excludes the +INF scores of padding refs)
        thr[st] = fminf(t, 3.4028234663852886e38f);
        if constexpr (LAZY) thrw[st] = thr[st] + bnd[st];
        if constexpr (PRE) {
            // A pair with a three-product score <= thr has 2 s^2 A <= thr + B8, A an integer: A <= floor((thr + B8) / (2 s^2)).
            // The fp32 sum, the product and inv2s2 itself are each within 2^-23 relative: 2^-20 of the magnitude and
            // one unit on top keep the rounding on the safe side (B8 carries two units for it).  Clamped below the
            // padding seeds, and far enough above INT_MIN for the conversion.
            const float w = (thr[st] + bnd[st]) * inv2s2;
            const float wu = w + fabsf(w) * 0x1p-20f + 1.0f;
            thrw8[st] = (int)fminf(fmaxf(floorf(wu), -(float)kI8PreThrMax), (float)kI8PreThrMax);
        }
    };
    // Slow path, step 2: one finished score x of ref j: append to the state's candidate ring (thr is finite
    // here — tighten clamps it — so "x <= thr" also excludes the +INF scores of padding refs).  `roomy`
    // (wave-uniform, computed once per slow tile): no lane of the wave is within a tile's worth of entries of
    // its ring's capacity, so the ring-wrap check — a load, hence a vmcnt wait that also drains the DMA ring —
    // is skipped by a scalar branch; it only runs on monotone inputs (every ref a new record).
    auto record = [&](auto st_c, float x, int j, bool roomy) __attribute__((always_inline)) {
        constexpr int st = decltype(st_c)::value;
        if (x <= thr[st]) {
            const unsigned off = loff + list_off(st) +
                                 (unsigned)(cnt[st] & (kCandCap - 1)) * (unsigned)(64 * sizeof(CandEntry));
            CandEntry *const dst = reinterpret_cast<CandEntry *>(lbase + off);
            if (__builtin_expect(!roomy, 0)) {
                // ring wrap: the slot's old entry may only be dropped if it is above the current
                // threshold (then it can never be within tau of the final minimum)
                if ((cnt[st] & kCandCountMask) >= kCandCap && dst->s <= thr[st]) cnt[st] |= kCandOverflow;
            }
            CandEntry e;
            e.s = x;
            e.j = j;
#if defined(NNS_DIAG) && defined(NNS_F_NOSTORE)   // timing experiment: the slow path without its global store
            asm volatile("" ::"v"(e.s), "v"(e.j), "v"(dst));
#else
            *dst = e;
#endif
            ++cnt[st];
        }
    };
    // minimum of the finished scores of one ref block for lane state st
    auto tile_min = [&](const typename OP::Acc &acc, auto st_c) __attribute__((always_inline)) -> float {
        constexpr int st = decltype(st_c)::value;
        if constexpr (T16) {
            const f32x4 &lo = acc.template at<0, st>();   // refs 4 g + i
            const f32x4 &hi = acc.template at<1, st>();   // refs 16 + 4 g + i
            const float t0 = fminf(fminf(lo[0], lo[1]), lo[2]);
            const float t1 = fminf(fminf(lo[3], hi[0]), hi[1]);
            return fminf(fminf(t0, t1), fminf(hi[2], hi[3]));
        } else {
            const f32x16 &t = acc.template at<st>();
            const float t0 = fminf(fminf(t[0], t[1]), t[2]);
            const float t1 = fminf(fminf(t[3], t[4]), t[5]);
            const float t2 = fminf(fminf(t[6], t[7]), t[8]);
            const float t3 = fminf(fminf(t[9], t[10]), t[11]);
            const float t4 = fminf(fminf(t[12], t[13]), t[14]);
            return fminf(fminf(fminf(t0, t1), t[15]), fminf(fminf(t2, t3), t4));
        }
    };
    auto frag_ptr = [&](const char *slot, int blk, int f) __attribute__((always_inline)) {
        if constexpr (L16) {
            // step F of the slot = block F / SPB, ref tile rt, k-step ks: the gathered operand (lazy16_gather)
            const int F = blk * SPB + f, rt = (F % SPB) / (SPB / 2), ks = F % (SPB / 2);
            return reinterpret_cast<const float4 *>(slot + (F / SPB) * BLK_BYTES) + (lazy16_gather(0, rt, ks) + lazy16_gather(lane, 0, 0));
        } else
        return (reinterpret_cast<const float4 *>(slot + (DEEP ? 0 : blk * BLK_BYTES)) + lane) + f * 64;
    };
    // slow path of one state: every score of the block against the lane's threshold
#ifdef NNS_DIAG
    unsigned diag_slow = 0, diag_tiles = 0;   // slow-path executions / retired (tile, state) pairs of this wave
    unsigned long long diag_cyc = 0;   // s_memtime ticks spent inside record_all (lazy: from the flag to the end of record_all)
    unsigned long long diag_sync = 0;  // s_memtime ticks spent inside sync_slot: the counted wait and the barrier
#endif
    auto record_all = [&](const typename OP::Acc &acc, int blk_global, auto st_c) __attribute__((always_inline)) {
        constexpr int st = decltype(st_c)::value;
#ifdef NNS_DIAG
        ++diag_slow;
        const unsigned long long diag_t0 = LAZY ? 0ull : __builtin_amdgcn_s_memtime();   // (lazy: timed from the flag, epilogue)
#endif
        // (the tile minimum is recomputed here, on the cold path, rather than kept live across the branch)
        const float tmv = tile_min(acc, st_c);
        tighten(st_c, tmv);
        // is any lane of the wave about to wrap its 64-entry ring (monotone inputs)?
        const bool roomy = __builtin_amdgcn_ballot_w64((cnt[st] & kCandCountMask) + 16 > kCandCap) == 0ull;
        if (a.tile_rec) {
            // TILE RECORDS (short ref streams).  A wave carries 32 queries per state and a query improves on its
            // t-th tile with probability ~1/t, so for the first ~32-64 tiles of a stream nearly EVERY tile takes
            // this path in some lane, and a stream of 256 tiles (1024 queries x 1 M refs: 128 splits) takes it on
            // a third of them — at the 16-deep tile, where a tile is 8 MFMAs, that was 40 % of the kernel.  Here
            // the path is short whatever the scores look like: the lane records the TILE — its minimum and the first
            // of the lane's 16 rows — and K5 evaluates V0's distance for those rows.  Completeness is unchanged:
            // a ref within tau of the final minimum makes its tile's minimum <= every threshold the lane ever holds.
            record(st_c, tmv, blk_global * 32 + 4 * h, roomy);
        } else if constexpr (T16) {
            const f32x4 &lo = acc.template at<0, st>();
            const f32x4 &hi = acc.template at<1, st>();
            const int jbase = blk_global * 32 + 4 * (lane >> 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) record(st_c, lo[r], jbase + r, roomy);
#pragma unroll
            for (int r = 0; r < 4; ++r) record(st_c, hi[r], jbase + 16 + r, roomy);
        } else {
            // Typically ONE lane has ONE score to append, and every instruction of this path delays the whole
            // workgroup at the next slot barrier: test the scores four at a time first (wave-uniform), descend
            // only into a group that has one.
            const f32x16 &t = acc.template at<st>();
            const int jbase = blk_global * 32 + 4 * h;
            // (the groups are tile_min's own triples + the sixteenth score: hipcc shares the group minima
            //  between the two, and with any other grouping it splits the hot path's v_min3 to do so —
            //  10 VALU instructions per retired tile instead of 8)
#pragma unroll
            for (int g = 0; g < 5; ++g) {
                const float gm = fminf(fminf(t[3 * g], t[3 * g + 1]), t[3 * g + 2]);
                if (__builtin_amdgcn_ballot_w64(gm <= thr[st]) != 0ull) {
#pragma unroll
                    for (int e = 0; e < 3; ++e) {
                        const int r = 3 * g + e;
                        record(st_c, t[r], jbase + (r & 3) + 8 * (r >> 2), roomy);
                    }
                }
            }
            if (__builtin_amdgcn_ballot_w64(t[15] <= thr[st]) != 0ull) record(st_c, t[15], jbase + 3 + 8 * 3, roomy);
        }
#ifdef NNS_DIAG
        if constexpr (!LAZY) diag_cyc += __builtin_amdgcn_s_memtime() - diag_t0;
#endif
    };
    // ---- record form 2 (fp32 32 x 32 tiles on short ref streams): the lane's TWO BEST TILES, branch-free ---------
    // A wave carries 32 queries per state and a query improves on its t-th tile with probability ~1/t, so on a stream
    // of a few hundred tiles a third of the tiles took the threshold test's slow path in SOME lane (335 195 of
    // 1 048 576 tile retirements at 1024 x 1 M x 16, ~800 cycles each with one record per tile, ~1400 with one per
    // score: profiles/r03_streams.txt) — at the 16-deep tile, where a tile is 8 MFMAs, a quarter of the kernel.
    // Short streams do not need lists at all: a lane keeps the minima of its best and second-best tile, where they
    // came from, and the minimum of the third-best — 3 compares + 7 selects behind the tile's 8 v_min3, in the
    // shadow of the SIMD partner's MFMAs, no branch, no store, no threshold.  At the end of the stream the lane writes
    // three entries.  K5 takes a = the minimum over the entries and evaluates V0's distance for the rows of every
    // recorded tile whose minimum is <= a + tau(a); if a lane's THIRD minimum is within the threshold too (three
    // tiles of one lane's stream within tau: duplicates, or refs packed closer than the filter resolves) the query
    // goes to the exact scan.  Completeness: tiles of a lane's stream with a minimum <= a + tau(a) are a prefix of
    // its tiles sorted by minimum — of length <= 2 unless the third is inside too.
    float m1[NS], m2[NS], m3[NS];
    int t1[NS], t2[NS];
#pragma unroll
    for (int st = 0; st < NS; ++st) {
        m1[st] = m2[st] = m3[st] = __builtin_inff();
        t1[st] = t2[st] = 0;
    }
    auto epilogue_top2 = [&](const typename OP::Acc &acc, int blk_global) __attribute__((always_inline)) {
        if constexpr (!T16) {
            static_for<NS>([&](auto st_c) __attribute__((always_inline)) {
                constexpr int st = decltype(st_c)::value;
                const float tm = tile_min(acc, st_c);
                // sorted insert of tm into m1 <= m2 <= m3 by v_med3 / v_min; the tile numbers follow with selects.
                // (The old values go through empty asm statements: a select between two elements of these arrays is
                //  otherwise rewritten by hipcc into a load through a selected POINTER, which keeps the arrays in scratch.)
                float o1 = m1[st], o2 = m2[st];
                int p1 = t1[st], p2 = t2[st];
                asm volatile("" : "+v"(o1), "+v"(o2), "+v"(p1), "+v"(p2));
                const bool lt1 = tm < o1, lt2 = tm < o2;   // strict: equal minima fill the next rank
                // (o1 <= o2 <= m3: the new second is the median of {tm, o1, o2}, the new third that of {tm, o2, m3}; scores
                //  are finite or +INF, never NaN: K2 routes NaN inputs to the exact kernels)
                m3[st] = __builtin_amdgcn_fmed3f(tm, o2, m3[st]);
                m2[st] = __builtin_amdgcn_fmed3f(tm, o1, o2);
                m1[st] = fminf(o1, tm);
                t2[st] = lt1 ? p1 : (lt2 ? blk_global : p2);
                t1[st] = lt1 ? blk_global : p1;
            });
        }
    };
    // record collection at the end of a ref block
    // (slot, blk: where the block's hi fragments still sit in the ring — the lazy form's refinement re-reads them)
    auto epilogue = [&](typename OP::Acc &acc, int blk_global, const char *slot, int blk) __attribute__((always_inline)) {
        if constexpr ((kAblate & 2) != 0) {   // diagnostic: keep the accumulators alive, collect nothing
            static_for<NS>([&](auto st_c) __attribute__((always_inline)) {
                constexpr int st = decltype(st_c)::value;
                if constexpr (T16) {
                    const f32x4 lo = acc.template at<0, st>(), hi = acc.template at<1, st>();
                    asm volatile("" ::"v"(lo), "v"(hi));
                } else {
                    const f32x16 t = acc.template at<st>();
                    asm volatile("" ::"v"(t));
                }
            });
            return;
        }
        if constexpr (T16) {
            // (16x16 tiles retire their ref tiles inside t16_step)
        } else {
            static_for<NS>([&](auto st_c) __attribute__((always_inline)) {
                constexpr int st = decltype(st_c)::value;
                const float tm = tile_min(acc, st_c);
#ifdef NNS_DIAG
                ++diag_tiles;
#endif
                if constexpr (LAZY) {
                    // tm is the minimum of the HI-HI scores; no three-product score of the tile is below tm - B, so a tile
                    // with tm > thr + B holds nothing within thr.  A flagged tile gets its cross products now, on the
                    // same accumulator: rh x ql from the ring slot, rl x qh from the lo region of the image (plain
                    // loads: the wait behind them also waits for older ring DMA pieces, as the !roomy branch's does)
                    if (__builtin_expect(__builtin_amdgcn_ballot_w64(tm <= thrw[st]) != 0ull, 0)) {
#ifdef NNS_DIAG
                        const unsigned long long diag_f0 = __builtin_amdgcn_s_memtime();   // flag .. end of record_all
#endif
                        const float4 *lo = reinterpret_cast<const float4 *>(a.rimg_lo) + (size_t)blk_global * (SPB * 64) + lane;
                        float4 rl[SPB];
#pragma unroll
                        for (int b = 0; b < SPB; ++b) rl[b] = lo[b * 64];
                        // (all of them in flight before the first is used: ONE round trip.  Left to itself hipcc rotates
                        //  two registers through load - wait - MFMA, a round trip per k-step, with the workgroup waiting
                        //  at the next slot barrier)
#pragma unroll
                        for (int b = 0; b < SPB; ++b) asm volatile("" : "+v"(rl[b].x), "+v"(rl[b].y), "+v"(rl[b].z), "+v"(rl[b].w));
                        static_for<SPB>([&](auto b_c) __attribute__((always_inline)) {
                            constexpr int b = decltype(b_c)::value;
                            const float4 rh = *frag_ptr(slot, blk, b);
                            acc.template at<st>() = OP::mma(rh, bq[st][2 * b + 1], acc.template at<st>());
                            acc.template at<st>() = OP::mma(rl[b], bq[st][2 * b], acc.template at<st>());
                        });
                        record_all(acc, blk_global, st_c);
#ifdef NNS_DIAG
                        diag_cyc += __builtin_amdgcn_s_memtime() - diag_f0;
#endif
                    }
                } else
                if (__builtin_expect(__builtin_amdgcn_ballot_w64(tm <= thr[st]) != 0ull, 0))   // rare: ~ln(n) tiles per lane
                    record_all(acc, blk_global, st_c);
            });
        }
    };
    auto mma_all = [&](typename OP::Acc &acc, const float4 &frag, auto b_c) __attribute__((always_inline)) {
        constexpr int b = decltype(b_c)::value;
        if constexpr (T16) {
            // (16x16 tiles go through t16_step)
        } else {
            if constexpr (LAZY) {
                // the fast path: ref hi fragment of k-step b x qh
                static_for<QB>([&](auto qc) __attribute__((always_inline)) {
                    constexpr int qb = decltype(qc)::value;
                    acc.template at<qb>() = OP::mma(frag, bq[qb][2 * b], acc.template at<qb>());
                });
            } else if constexpr (OP::kSplit) {
                // ref hi fragment x (qh, ql) of the k-step; ref lo fragment x qh
                static_for<QB>([&](auto qc) __attribute__((always_inline)) {
                    constexpr int qb = decltype(qc)::value;
                    if constexpr (b % 2 == 0) {
                        acc.template at<qb>() = OP::mma(frag, bq[qb][b], acc.template at<qb>());
                        acc.template at<qb>() = OP::mma(frag, bq[qb][b + 1], acc.template at<qb>());
                    } else {
                        acc.template at<qb>() = OP::mma(frag, bq[qb][b - 1], acc.template at<qb>());
                    }
                });
            } else {
                static_for<QB>([&](auto qc) __attribute__((always_inline)) {
                    constexpr int qb = decltype(qc)::value;
                    acc.template at<qb>() = OP::mma(frag, bq[qb][b], acc.template at<qb>());
                });
            }
        }
    };

    // ---- 16x16 tiles: one step, with the other ref tile's record collection folded in --------
    constexpr int NT16 = T16 ? NS : 4;
    float tmh[NT16];   // minima of the retiring ref tile, one per state
    int tmi[NT16];     // (pre-pass: the integer minima)
    unsigned long long hm[NT16];
#pragma unroll
    for (int i = 0; i < NT16; ++i) {
        tmh[i] = 0.0f;
        tmi[i] = 0;
        hm[i] = 0ull;
    }
    // threshold test of the retiring ref tile ot of block oblk: ONE wave-uniform branch for the
    // common case (no lane has a record in any of its four states), then per state inside
    // (oslot, oin: where the retiring tile's block still sits in the ring — the lazy form's refinement re-reads its hi
    //  fragments)
    auto t16_test = [&](typename OP::Acc &acc, int oblk, auto ot_c, const char *oslot, int oin) __attribute__((always_inline)) {
        if constexpr (T16) {
            constexpr int ot = decltype(ot_c)::value;
            unsigned long long any = 0ull;
#pragma unroll
            for (int i = 0; i < NT16; ++i) any |= hm[i];
#ifdef NNS_DIAG
            diag_tiles += NT16;
#endif
            if constexpr (PRE) {
                // PRE-PASS: a flagged (ref tile, state) — some lane's integer minimum within thrw8 — gets the three-product
                // scores of its 16 x 16 pairs on a fresh accumulator: lazy16's chain in lazy16's order (the norms as srcC of
                // the first rh.qh MFMA, the other three, then rh.ql and rl.qh per k-step), so a refined score has the bits
                // lazy16 gives it.  Nothing of it is in the ring: rh, rl out of the image's hi and lo regions, qh, ql out
                // of the query image (all through lazy16_gather), the four norms out of rnorm.
                // oslot / oin MUST STAY UNUSED here: pre_cadence_ok and the kernel's static_assert rest on an interval reading
                // its own and the next slot only.  A refinement that re-read the retiring tile's slot (s - 1, as lazy16's does)
                // would need AHEAD + G < ring depth instead of <=: tools/pre_cadence_check.cpp models that too (reads_prev).
                (void)oslot, (void)oin;
                // (the very first tests of a stream see the start accumulators / no masks: nothing there)
                const bool refine = (any != 0ull) & (oblk >= slot0 * BPS);
                if (__builtin_expect(refine, 0)) {   // cold: laid out off the MFMA stream
                    constexpr int NK = 4;   // k-steps of 32 dims of the bf16 chain at KT = 128
                    const float4 *hi = reinterpret_cast<const float4 *>(a.rimg) + (size_t)oblk * (2 * NK * 64);
                    const float4 *lo = reinterpret_cast<const float4 *>(a.rimg_lo) + (size_t)oblk * (2 * NK * 64);
                    const int jbase = oblk * 32 + 16 * ot + 4 * g16;
                    static_for<NT16>([&](auto st_c) __attribute__((always_inline)) {
                        constexpr int st = decltype(st_c)::value;
                        if (hm[st] != 0ull) {
#ifdef NNS_DIAG
                            ++diag_slow;
                            const unsigned long long diag_f0 = __builtin_amdgcn_s_memtime();
#endif
                            const float4 *qs = a.qimg + (size_t)(qblk0 + (st >> 1)) * (QFB * 64);
                            // (every load is issued AND consumed inside the state's branch, all of them in flight before
                            //  the first is used: see the lazy16 refinement below)
                            // (the ref-side loads once per flagged TILE instead, ahead of the states, measured within the
                            //  run-to-run spread of this form at C3 and was dropped: DESIGN, "Barrier cadence of the pre-pass")
                            float4 rh[NK], rl[NK], qh[NK], ql[NK];
                            const float4 nv = *reinterpret_cast<const float4 *>(a.rnorm + jbase);
#pragma unroll
                            for (int ks = 0; ks < NK; ++ks) rh[ks] = hi[lazy16_gather(lane, ot, ks)];
#pragma unroll
                            for (int ks = 0; ks < NK; ++ks) qh[ks] = qs[lazy16_gather(lane, st & 1, ks, 2, 0)];
#pragma unroll
                            for (int ks = 0; ks < NK; ++ks) rl[ks] = lo[lazy16_gather(lane, ot, ks)];
#pragma unroll
                            for (int ks = 0; ks < NK; ++ks) ql[ks] = qs[lazy16_gather(lane, st & 1, ks, 2, 1)];
#pragma unroll
                            for (int ks = 0; ks < NK; ++ks) {
                                asm volatile("" : "+v"(rh[ks].x), "+v"(rh[ks].y), "+v"(rh[ks].z), "+v"(rh[ks].w));
                                asm volatile("" : "+v"(qh[ks].x), "+v"(qh[ks].y), "+v"(qh[ks].z), "+v"(qh[ks].w));
                                asm volatile("" : "+v"(rl[ks].x), "+v"(rl[ks].y), "+v"(rl[ks].z), "+v"(rl[ks].w));
                                asm volatile("" : "+v"(ql[ks].x), "+v"(ql[ks].y), "+v"(ql[ks].z), "+v"(ql[ks].w));
                            }
                            f32x4 o = {nv.x, nv.y, nv.z, nv.w};
#pragma unroll
                            for (int ks = 0; ks < NK; ++ks) o = OP::mma16_bf16(rh[ks], qh[ks], o);
#pragma unroll
                            for (int ks = 0; ks < NK; ++ks) {
                                o = OP::mma16_bf16(rh[ks], ql[ks], o);
                                o = OP::mma16_bf16(rl[ks], qh[ks], o);
                            }
                            tighten(st_c, fminf(fminf(fminf(o[0], o[1]), o[2]), o[3]));
                            // (two lists per query, the lanes with even g own them: the hand-over of the lazy16 refinement)
                            const bool roomy = __builtin_amdgcn_ballot_w64((cnt[st] & kCandCountMask) + 8 > kCandCap) == 0ull;
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const unsigned ob = __float_as_uint(o[r]);
                                const auto sw = __builtin_amdgcn_permlane16_swap(ob, ob, false, false);
                                record(st_c, owner ? o[r] : __builtin_inff(), jbase + r, roomy);
                                record(st_c, owner ? __uint_as_float(sw[1]) : __builtin_inff(), jbase + 4 + r, roomy);
                            }
#ifdef NNS_DIAG
                            diag_cyc += __builtin_amdgcn_s_memtime() - diag_f0;
#endif
                        }
                    });
                }
            } else if constexpr (L16) {
                // LAZY: a flagged (ref tile, state) — some lane's hi-hi minimum within fl(thr + B) — gets its cross products
                // now, on the same accumulator: rh x ql and rl x qh per k-step, rh out of the ring, rl and ql plain global
                // loads through the gather (rl: the lo region of the image; ql: the query image, 16 KiB per wave, L2).
                // The retiring tile may be the last one of the PREVIOUS slot: the partners run in lock-step, so during
                // interval s every wave is in interval s, and the only DMA issued fills slot s + AHEAD, which is slot
                // s - 1's ring position only if AHEAD + 1 is a multiple of the ring depth.
                static_assert(!OP::kLag && (AHEAD + 1) % F_D<OP> != 0, "slot s - 1 is not refilled during interval s");
                // (the very first retirement of a stream is of the +INF start accumulators: nothing there, and no slot)
                // (one condition, not a short-circuit pair: hipcc lays a pair out with the cold side falling through)
                const bool refine = (any != 0ull) & (oblk >= slot0 * BPS);
                if (__builtin_expect(refine, 0)) {   // cold: laid out off the MFMA stream
                    constexpr int NKS = SPB / 2;
                    const float4 *lo = reinterpret_cast<const float4 *>(a.rimg_lo) + (size_t)oblk * (SPB * 64);
                    const int jbase = oblk * 32 + 16 * ot + 4 * g16;
                    static_for<NT16>([&](auto st_c) __attribute__((always_inline)) {
                        constexpr int st = decltype(st_c)::value;
                        if (hm[st] != 0ull) {
#ifdef NNS_DIAG
                            ++diag_slow;
                            const unsigned long long diag_f0 = __builtin_amdgcn_s_memtime();
#endif
                            const float4 *qs = a.qimg + (size_t)(qblk0 + (st >> 1)) * (QFB * 64);
                            // (every load is issued AND consumed inside the state's branch — a second flagged state of the
                            //  tile reads rl and rh again: a load left in flight where the branch rejoins the slot loop makes
                            //  hipcc wait with vmcnt(0) in the loop, in front of the first fragment read that reuses a register)
                            float4 rl[NKS], rh[NKS], ql[NKS];
#pragma unroll
                            for (int ks = 0; ks < NKS; ++ks) rl[ks] = lo[lazy16_gather(lane, ot, ks)];
#pragma unroll
                            for (int ks = 0; ks < NKS; ++ks) ql[ks] = qs[lazy16_gather(lane, st & 1, ks, 2, 1)];
#pragma unroll
                            for (int ks = 0; ks < NKS; ++ks) rh[ks] = *frag_ptr(oslot, oin, ot * NKS + ks);
                            // (all of them in flight before the first is used: ONE round trip, see filter_lazy_kernel)
#pragma unroll
                            for (int ks = 0; ks < NKS; ++ks) {
                                asm volatile("" : "+v"(rl[ks].x), "+v"(rl[ks].y), "+v"(rl[ks].z), "+v"(rl[ks].w));
                                asm volatile("" : "+v"(ql[ks].x), "+v"(ql[ks].y), "+v"(ql[ks].z), "+v"(ql[ks].w));
                            }
                            f32x4 &o = acc.template at<ot, st>();
#pragma unroll
                            for (int ks = 0; ks < NKS; ++ks) {
                                OP::mma16(rh[ks], ql[ks], o);
                                OP::mma16(rl[ks], bq[st][ks], o);
                            }
                            // asm MFMAs: the compiler adds no wait states in front of the VALU reads below
                            asm volatile("s_nop 7" : "+v"(o));
                            tighten(st_c, fminf(fminf(fminf(o[0], o[1]), o[2]), o[3]));
                            // Two lists per query: the lanes with even g own them, and lane g ^ 1 hands over its four scores
                            // (rows 4 (g ^ 1) ..) through a row swap: on an even row, word 1 of swap(x, x) is x of lane + 16.
                            // The owner tests all eight against its own threshold (tighten: any of the query's lanes' is
                            // valid, and they have just adopted the smallest); the other lanes append nothing.
                            const bool roomy = __builtin_amdgcn_ballot_w64((cnt[st] & kCandCountMask) + 8 > kCandCap) == 0ull;
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const unsigned ob = __float_as_uint(o[r]);
                                const auto sw = __builtin_amdgcn_permlane16_swap(ob, ob, false, false);
                                record(st_c, owner ? o[r] : __builtin_inff(), jbase + r, roomy);
                                record(st_c, owner ? __uint_as_float(sw[1]) : __builtin_inff(), jbase + 4 + r, roomy);
                            }
#ifdef NNS_DIAG
                            diag_cyc += __builtin_amdgcn_s_memtime() - diag_f0;
#endif
                        }
                    });
                }
            } else
            if (__builtin_expect(any != 0ull, 0)) {   // cold: laid out off the MFMA stream
                const int jbase = oblk * 32 + 16 * ot + 4 * (lane >> 4);
                static_for<NT16>([&](auto st_c) __attribute__((always_inline)) {
                    constexpr int st = decltype(st_c)::value;
                    if (hm[st] != 0ull) {
                        const f32x4 &o = acc.template at<ot, st>();
                        tighten(st_c, tmh[st]);
                        const bool roomy = __builtin_amdgcn_ballot_w64((cnt[st] & kCandCountMask) + 4 > kCandCap) == 0ull;
                        if (a.tile_rec) {   // one record for the lane's four rows of this 16-ref tile (see record_all)
                            record(st_c, tmh[st], jbase, roomy);
                        } else {
#pragma unroll
                            for (int r = 0; r < 4; ++r) record(st_c, o[r], jbase + r, roomy);
                        }
                    }
                });
            }
        }
    };
    // the four states' lane masks "this lane has a score within its threshold" (v_cmp straight to
    // SGPR pairs, computed a step before the branch that reads them)
    auto t16_masks = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int st = 0; st < NT16; ++st) {
            if constexpr (PRE) hm[st] = __builtin_amdgcn_ballot_w64(tmi[st] <= thrw8[st]);
            else hm[st] = __builtin_amdgcn_ballot_w64(tmh[st] <= (LAZY ? thrw[st] : thr[st]));
        }
    };
    // step b = 8 rt + ks of the block blk_global: the 4 MFMAs of ref tile rt's k-step ks; at
    // ks = 1 the other tile's four accumulators (finished at its k-step 7, >= 5 MFMAs ago) are
    // reduced, two v_min behind each MFMA; at ks = 2 they are tested.  The other tile of rt = 0
    // is tile 1 of the PREVIOUS block (kernel start: +INF accumulators, nothing to record).
    auto t16_step = [&](typename OP::Acc &acc, const float4 &frag, int blk_global, auto b_c, const char *oslot, int oin) __attribute__((always_inline)) {
        if constexpr (T16) {
            constexpr int b = decltype(b_c)::value;
            constexpr int NKS = SPB / 2;              // k-steps of 32 dims per 16-ref tile
            // (with two query tiles per wave a step is two MFMAs: retire one k-step later, so that the reads of the other
            //  tile's accumulators still sit >= 5 MFMAs behind the MFMAs that finished them)
            constexpr int RET = NT16 >= 4 ? 1 : 2;
            // (the pre-pass refines on a fresh accumulator: the retiring tile may be tested while it is seeded again, at
            //  its own k-step 0, a step behind its minima and masks)
            static_assert(NKS >= RET + 2 || (PRE && NKS == RET + 1), "the other tile is retired at k-steps RET and RET + 1");
            constexpr int rt = b / NKS, ks = b % NKS, ot = 1 - rt;
            static_for<NT16>([&](auto qc) __attribute__((always_inline)) {
                constexpr int qt = decltype(qc)::value;
                if constexpr (ks == 0) OP::mma16_seed(frag, bq[qt][0], acc.template at<rt, qt>(), rt == 0 ? nseed0 : nseed1);
                else OP::mma16(frag, bq[qt][ks], acc.template at<rt, qt>());
                if constexpr (ks == RET) {
                    // Name the retiring tile's accumulator as ONE in/out tuple before its elements are read:
                    // without it hipcc carries elements 1 and 3 of each tile across the loop back-edge in
                    // separate registers (8 v_mov at the latch, 8 more to put them back in front of the tile's
                    // seed MFMA, whose in/out constraint "reads" them): 16 of the 74 VALU instructions of an
                    // interval, in a loop where every VALU issue cycle is an MFMA issue cycle lost.
                    asm volatile("" : "+v"(acc.template at<ot, qt>()));
                    // (OpI8: the retiring tile's i32 dot products become its fp32 scores here, under its own norms)
                    if constexpr (OP::kI8) OP::retire(acc.template at<ot, qt>(), ot == 0 ? nseed0 : nseed1);
                    const f32x4 o = acc.template at<ot, qt>();
                    if constexpr ((kAblate & 2) != 0) asm volatile("" ::"v"(o));
                    else if constexpr (PRE) {
                        const i32x4 oi = __builtin_bit_cast(i32x4, o);
                        tmi[qt] = min(min(min(oi[0], oi[1]), oi[2]), oi[3]);
                    }
                    else tmh[qt] = fminf(fminf(fminf(o[0], o[1]), o[2]), o[3]);
                    __builtin_amdgcn_sched_barrier(0);   // keep the pair right behind its MFMA
                }
            });
            if constexpr (ks == RET && (kAblate & 2) == 0) t16_masks();
            if constexpr (PRE) {
                // (k-step 0 of tile rt: the masks of the step before are tile rt's own, of the block before this one)
                if constexpr (ks == 0 && (kAblate & 2) == 0) t16_test(acc, blk_global - 1, std::integral_constant<int, rt>{}, oslot, oin);
            } else
            if constexpr (ks == RET + 1 && (kAblate & 2) == 0) t16_test(acc, rt == 0 ? blk_global - 1 : blk_global, std::integral_constant<int, ot>{}, oslot, oin);
        }
    };

    // ---- the software pipeline of one barrier interval -----------------------------------
    // An interval is the 32 fragment steps of one ring slot (BPS image blocks x SPB fragments;
    // one step = one ds_read_b128 + its MFMAs for the wave's query blocks).  Waves 0..3
    // (LAG = 0) run the slot's blocks in order; waves 4..7 (LAG = 1) run HALF A BLOCK behind
    // (they start each interval with the second half of the previous slot's last block), so
    // one SIMD partner's tile boundary (epilogue, accumulator re-seed from the norms) falls in
    // the middle of the other's MFMA chain.  Fragments are prefetched PF steps ahead through
    // a register ring that is carried ACROSS the barrier: the LDS ring is 4 slots deep and the
    // barrier of interval s confirms slot s + 1, so the first fragments of interval s + 1 are
    // already in flight when its barrier releases and the MFMA chain restarts at once.
    constexpr int PF = OP::kPrefetch;
    constexpr int RING = PF < 4 ? 4 : 8;
    constexpr int LAGOFF = SPB / 2;
    static_assert(PF < RING && SPS % RING == 0 && (!OP::kLag || PF <= LAGOFF), "prefetch ring");
    typename OP::Acc acc;
    if constexpr (T16) {
        // (OpI8: i32 zeros, retired under the norm +INF — see nseed1)
        // (OpI8Pre: the padding seed's bits, an integer above every threshold)
        const float inf0 = OP::kI8 ? 0.0f : PRE ? __int_as_float(kI8PrePadSeed) : __builtin_inff();
        const f32x4 inf4 = {inf0, inf0, inf0, inf0};
        static_for<NT16>([&](auto qc) __attribute__((always_inline)) {
            acc.template at<0, decltype(qc)::value>() = inf4;
            acc.template at<1, decltype(qc)::value>() = inf4;
        });
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc.v0[r] = acc.v1[r] = __builtin_inff();
    }
    float4 fr[RING];

    using I0c = std::integral_constant<int, 0>;
    using I1c = std::integral_constant<int, 1>;
    // s: slot index relative to slot0; cur/prev/nxt: ring images of slots s, s-1, s+1
    auto interval = [&](auto lag_c, auto dph_c, auto half_c, auto rec_c, int s, const char *cur, const char *prev, const char *nxt) __attribute__((always_inline)) {
        constexpr int LAG = decltype(lag_c)::value;
        constexpr int REC2 = decltype(rec_c)::value;   // 1: record form 2 (the lane's two best tiles), 32 x 32 tiles only
        constexpr int DPH = decltype(dph_c)::value;   // DMA phase: the SIMD partners issue at different steps
        constexpr int HALF = decltype(half_c)::value; // blocks spanning two slots: which of them this interval is
        const bool first = s == 0;
        // first block of this slot (shallow) / of this slot's super-period (deep: slot0 and ns are whole super-periods)
        const int blk0_global = SPBLK == 1 ? (slot0 + s) * BPS : (slot0 + s) / SUP_SLOTS * SUP_BLKS;
        // compile-time schedule: step t works on position u = t - LAG * LAGOFF of the slot's
        // fragment stream (u < 0: tail of the previous slot; u >= 32: head of the next one)
        auto load = [&](auto tc_) __attribute__((always_inline)) {
            constexpr int t = decltype(tc_)::value;
            constexpr int u = t - LAG * LAGOFF;
            // (fragment u of a slot sits at u KiB whatever the block depth: block * SPB + step = u)
            if constexpr (u < 0) fr[t % RING] = *frag_ptr(prev, 0, SPS + u);
            else if constexpr (u < SPS) fr[t % RING] = *frag_ptr(cur, 0, u);
            else fr[t % RING] = *frag_ptr(nxt, 0, u - SPS);   // (last interval: stale slot, unused)
        };
        static_for<SPS>([&](auto tc_) __attribute__((always_inline)) {
            constexpr int t = decltype(tc_)::value;
            constexpr int u = t - LAG * LAGOFF;
            // block (of the slot / of the super-period) and operand / k position inside it
            constexpr int blk = SPBLK == 1 ? (u < 0 ? BPS - 1 : u / SPB) : (32 * HALF + u) / SPB;
            constexpr int b = SPBLK == 1 ? (u < 0 ? SPB + u : u % SPB) : (32 * HALF + u) % SPB;
            load(std::integral_constant<int, t + PF>{});
            // one DMA piece per step, two slots ahead, in the MFMA shadow, at different steps
            // for the two SIMD partners (an LDS-DMA issue stalls the issuing wave ~100 cycles;
            // past the end of the shard it reads the image's padding)
            if constexpr ((kAblate & 16) == 0) {
                constexpr int d0 = DPH == 0 ? 2 : SPS / 2;
                // steps between pieces: two where they fit — except K4's 256-deep 16x16x32 form, whose pieces go out on consecutive
                // steps (same-device A/B on C5: 78.2 -> 77.5 ms, +0.9 %; the 512- / 384-deep tiles lose 1 % that way, three steps
                // apart loses everywhere: profiles/r03_ab_dma_burst.txt)
                constexpr int sp = (T16 && SPB == 16) ? 1 : ((F_PPW + F_NP) * 2 <= 14 ? 2 : 1);
                static_assert(d0 + sp * (F_PPW + F_NP) <= SPS, "DMA pieces must fit the interval");
                // fp32 operators issue a slot's pieces BACK TO BACK at one step (round 3, second session): a lone LDS-DMA piece
                // costs its SIMD ~130 cycles of MFMA issue, a burst of them far less per piece (tools/ubench/chain_loop.hip:
                // 36.8 -> 25.2 ms); C3 118.3 -> 117.6 ms (OP::kDmaBurst: by tile depth).  The bf16 operators keep one piece per step: bursts cost THEM 1 - 6 %
                // (profiles/r03_ab_dma_burst.txt) — their intervals are 8 - 16x shorter and a burst stalls the lock-step partner too.
                if constexpr (OP::kDmaBurst) {
                    if constexpr (t == d0) issue(s + AHEAD);
                } else if constexpr (t >= d0 && t < d0 + sp * (F_PPW + F_NP) && (t - d0) % sp == 0) {
                    issue_piece(s + AHEAD, (t - d0) / sp);
                }
            }
            if constexpr (T16) {
                // norms two steps ahead: tile 1 of this block; tile 0 of the next block (next ring
                // slot after the slot's last block: confirmed by this interval's barrier)
                if constexpr (b == SPB / 2 - 2) seed16(cur, blk, I1c{});
                if constexpr (b == SPB - 2) seed16(blk + 1 < BPS ? cur : nxt, (blk + 1) % BPS, I0c{});
            } else if constexpr (b == 0) {   // a tile is seeded right where it starts
                if constexpr (kSeedAhead) {
                    seed_apply(acc);   // (read a tile ago; the next tile's: block blk + 1 of this slot, or the next slot's first —
                    seed_fetch(blk + 1 < BPS ? cur : nxt, (blk + 1) % BPS);   // landed and confirmed by this interval's barrier)
                } else {
                    seed(acc, cur, blk);
                }
            }
            // (LAG 1, very first interval: its first LAGOFF steps chew on a not-yet-written ring
            //  slot; that accumulator is discarded below and re-seeded at the next tile)
            if constexpr (T16) {
                // (the tile retired during ref tile 0's steps is tile 1 of the block before: the previous slot's last at blk 0)
                constexpr bool oprev = b < SPB / 2 && blk == 0;
                t16_step(acc, fr[t % RING], blk0_global + blk, std::integral_constant<int, b>{}, oprev ? prev : cur,
                         oprev ? BPS - 1 : (b < SPB / 2 ? blk - 1 : blk));
            } else {
                mma_all(acc, fr[t % RING], std::integral_constant<int, b>{});
                if constexpr (b == SPB - 1) {                // the tile's epilogue right at its end
                    if constexpr (REC2) {   // (a first interval's lagging half block chewed on garbage: skipped like below)
                        if constexpr (u < 0) {
                            if (!first) epilogue_top2(acc, blk0_global - 1);
                        } else {
                            epilogue_top2(acc, blk0_global + blk);
                        }
                    } else if constexpr (u < 0) {
                        if (!first) epilogue(acc, blk0_global - 1, prev, BPS - 1);
                    } else {
                        epilogue(acc, blk0_global + blk, cur, blk);
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        });
    };

    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    const bool half = wave >= F_NW / 2;   // wave-uniform: the second wave of each SIMD
#ifdef NNS_F_NOLAG
    const bool lag = false;   // diagnostic: SIMD partners in lock-step
#else
    const bool lag = OP::kLag && half;
#endif
    auto ring = [&](int s) __attribute__((always_inline)) { return smem + ((s + F_D<OP>) & (F_D<OP> - 1)) * F_SLOT_BYTES<OP>; };
    static_assert((F_D<OP> & (F_D<OP> - 1)) == 0, "ring depth must be a power of two");

    // prologue: slots 0 .. AHEAD - 1 in flight; confirm slot 0 (a cadence of G: slots 0 .. G, what the first group reads);
    // start interval 0's first fragments
    // (with G > 1 interval 0's sync_slot then waits on the same count with nothing issued in between: redundant by design —
    //  only slot 0 is read before it — so that every loop barrier, the first included, finds its G slots confirmed the same way)
    static_for<AHEAD>([&](auto s_c) __attribute__((always_inline)) { issue(decltype(s_c)::value); });
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((G == 1 ? AHEAD - 1 : AHEAD - G - 1) * F_PPS) : "memory");
    __builtin_amdgcn_s_barrier();
    if constexpr (T16) seed16(ring(0), 0, I0c{});   // the first block's tile-0 norms
    seed_fetch(ring(0), 0);                          // (shallow lock-step tiles: the first tile's norms)
    // (LAG 1 reads ring slot -1 here: garbage in, discarded — see the interval)
    static_for<PF>([&](auto t) __attribute__((always_inline)) {
        constexpr int tt = decltype(t)::value;
        if constexpr (OP::kLag) {
            if (lag) fr[tt % RING] = *frag_ptr(ring(-1), BPS - 1, SPB - LAGOFF + tt);
            else fr[tt % RING] = *frag_ptr(ring(0), 0, tt);
        } else {
            fr[tt % RING] = *frag_ptr(ring(0), 0, tt);   // (slot-local fragment tt)
        }
    });
    // The slot loop, one copy per interval variant (the dispatch is wave-uniform and loop-invariant): with
    // the three variants as branches inside ONE loop, hipcc parks the accumulators in different register
    // tuples at the merge and at the loop header and reconciles them with ~48 v_mov at every back-edge.
    // Every wave executes the same barriers whichever copy it runs: one per interval (OpI8Pre: one per group of G).
    auto slot_loop = [&](auto lag_c, auto dph_c, auto rec_c) __attribute__((always_inline)) {
        auto sync_slot = [&]() __attribute__((always_inline)) {
            if constexpr ((kAblate & 1) == 0) {
#ifdef NNS_DIAG
                const unsigned long long diag_s0 = __builtin_amdgcn_s_memtime();
#endif
                // my share of slot s+1 has landed.  AHEAD 2: issued an interval ago, the only DMA in flight.  AHEAD 3:
                // issued two intervals ago; the F_PPS pieces of slot s+2 issued since stay in flight (vmcnt counts
                // in issue order; a candidate store of the slow path issued in between only makes the wait longer)
                // (a cadence of G: my share of slots s+1 .. s+G, the rest of the group and the slot its last interval
                //  prefetches from; slots s+G+1 .. s+AHEAD-1 stay in flight)
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"((AHEAD - G - 1) * F_PPS) : "memory");
                // everyone's share of slot s+1 has landed; everyone is done with slot s-2
                // (a cadence of G: everyone's share of slots s+1 .. s+G has landed; everyone is done with every slot before s)
                __builtin_amdgcn_s_barrier();
#ifdef NNS_DIAG
                diag_sync += __builtin_amdgcn_s_memtime() - diag_s0;
#endif
            }
        };
        if constexpr (SPBLK == 2) {
            // a block = two slots (ns is even: filter_plan): even slot = k-steps 0..31, odd slot = 32..63
            for (int s = 0; s < ns; s += 2) {
                sync_slot();
                interval(lag_c, dph_c, I0{}, rec_c, s, ring(s), ring(s - 1), ring(s + 1));
                sync_slot();
                interval(lag_c, dph_c, I1{}, rec_c, s + 1, ring(s + 1), ring(s), ring(s + 2));
            }
        } else if constexpr (SPBLK > 2) {
            // a super-period of SPBLK slots (ns is a multiple of it: filter_plan) — 48-step blocks: A 0..31 | A 32..47,
            // B 0..15 | B 16..47; 40-step blocks: four blocks over five slots
            for (int s = 0; s < ns; s += SPBLK) {
                static_for<SPBLK>([&](auto ph_c) __attribute__((always_inline)) {
                    constexpr int ph = decltype(ph_c)::value;
                    sync_slot();
                    interval(lag_c, dph_c, ph_c, rec_c, s + ph, ring(s + ph), ring(s + ph - 1), ring(s + ph + 1));
                });
            }
        } else {
            for (int s = 0; s < ns; ++s) {
                // (the predicate is a function of s alone: every wave executes the same barriers, ceil(ns / G) of them,
                //  wherever its refinements fall; the branch is scalar and the loop stays one interval per iteration)
                if constexpr (G == 1) sync_slot();
                else if (s % G == 0) sync_slot();
                interval(lag_c, dph_c, I0{}, rec_c, s, ring(s), ring(s - 1), ring(s + 1));
                if constexpr (!OP::kLag) {
                    // lock-step partners (staggering only their DMA issue steps, or packing / spreading the
                    // pieces differently, measured +-0.5 % on C5).  The interval ends on the MFMAs that finish
                    // ref tile 1, which is retired in the NEXT interval: hipcc is free to split / copy those
                    // accumulators at the loop back-edge (it did: v_mov of single elements right behind the
                    // MFMAs = stale reads).  Whatever it does with them now happens behind the 8 wait states
                    // their readers need.
#ifndef NNS_F_NOLATCHFENCE   // (timing experiments only: without it the results are wrong)
                    if constexpr (T16) OP::mma16_tail_fence(acc);
#endif
                }
            }
        }
    };
    // (the record form, like the interval variant, is wave-uniform and loop-invariant: one copy of the loop each)
    const bool top2 = !T16 && a.tile_rec == 2;
    if constexpr (OP::kLag) {
        if (top2) {
            if (!half) slot_loop(I0{}, I0{}, I1{});
            else if (lag) slot_loop(I1{}, I1{}, I1{});
            else slot_loop(I0{}, I1{}, I1{});
        } else {
            if (!half) slot_loop(I0{}, I0{}, I0{});
            else if (lag) slot_loop(I1{}, I1{}, I0{});
            else slot_loop(I0{}, I1{}, I0{});
        }
    } else if constexpr (!T16) {
        if (top2) slot_loop(I0{}, I0{}, I1{});
        else slot_loop(I0{}, I0{}, I0{});
    } else {
        slot_loop(I0{}, I0{}, I0{});
    }
    if constexpr (T16) {   // ref tile 1 of the last block is still to be retired
        OP::mma16_tail_fence(acc);
        if constexpr (PRE && (kAblate & 2) == 0) {
            // the last block's tile 0 has its masks (k-step 1 of tile 1) and no seed step to be tested at; then tile 1
            t16_test(acc, (slot0 + ns) * BPS - 1, std::integral_constant<int, 0>{}, ring(ns - 1), BPS - 1);
            static_for<NT16>([&](auto qc) __attribute__((always_inline)) {
                const i32x4 oi = __builtin_bit_cast(i32x4, acc.template at<1, decltype(qc)::value>());
                tmi[decltype(qc)::value] = min(min(min(oi[0], oi[1]), oi[2]), oi[3]);
            });
            t16_masks();
            t16_test(acc, (slot0 + ns) * BPS - 1, std::integral_constant<int, 1>{}, ring(ns - 1), BPS - 1);
        } else
        if constexpr ((kAblate & 2) == 0) {
            static_for<NT16>([&](auto qc) __attribute__((always_inline)) {
                if constexpr (OP::kI8) OP::retire(acc.template at<1, decltype(qc)::value>(), nseed1);
                const f32x4 &o = acc.template at<1, decltype(qc)::value>();
                tmh[decltype(qc)::value] = fminf(fminf(fminf(o[0], o[1]), o[2]), o[3]);
            });
            t16_masks();
            t16_test(acc, (slot0 + ns) * BPS - 1, std::integral_constant<int, 1>{}, ring(ns - 1), BPS - 1);
        }
    }
    if constexpr (OP::kLag) if (lag) {   // the lagging half block of the last slot; its first PF fragments are in the ring
        const char *lastp = ring(ns - 1);
        static_for<LAGOFF>([&](auto tc_) __attribute__((always_inline)) {
            constexpr int t = decltype(tc_)::value;
            if constexpr (t + PF < LAGOFF) fr[(t + PF) % RING] = *frag_ptr(lastp, BPS - 1, SPB - LAGOFF + t + PF);
            mma_all(acc, fr[t % RING], std::integral_constant<int, SPB - LAGOFF + t>{});
        });
        if (top2) epilogue_top2(acc, (slot0 + ns) * BPS - 1);
        else epilogue(acc, (slot0 + ns) * BPS - 1, lastp, BPS - 1);
    }
    if constexpr (!T16) if (top2) {
        // record form 2: three entries per lane state — (best tile's minimum, first ref of the lane's rows of that tile),
        // the same for the second best, and the third-best minimum alone (K5: within the threshold = exact scan)
#pragma unroll
        for (int st = 0; st < NS; ++st) {
            CandEntry *const dst = reinterpret_cast<CandEntry *>(lbase + loff + (unsigned)(st * (kCandCap * 64 * (int)sizeof(CandEntry))));
            CandEntry e;
            e.s = m1[st];
            e.j = t1[st] * 32 + 4 * h;
            dst[0] = e;
            e.s = m2[st];
            e.j = t2[st] * 32 + 4 * h;
            dst[64] = e;
            e.s = m3[st];
            e.j = 0;
            dst[128] = e;
            cnt[st] = 3;
        }
    }
#pragma unroll
    for (int st = 0; st < NS; ++st) {
        if constexpr (Q2) {
            if (owner) a.counts[(lblk0 + (st >> 1)) * 64 + 32 * (g16 >> 1) + 16 * (st & 1) + i16] = cnt[st];
        } else {
            a.counts[(lblk0 + st) * 64 + lane] = cnt[st];
        }
    }
#ifdef NNS_DIAG
    if (a.stamps && lane == 0) {   // totals behind the per-workgroup stamps
        unsigned long long *tot = a.stamps + 4 * (size_t)gridDim.x * gridDim.y;
        atomicAdd(tot, (unsigned long long)diag_slow);
        atomicAdd(tot + 1, (unsigned long long)diag_tiles);
        atomicAdd(tot + 2, diag_cyc);
        atomicAdd(tot + 3, diag_sync);
        atomicAdd(tot + 4, 1ull);   // (waves)
    }
    if (a.stamps && threadIdx.x == 0) {
        unsigned long long *o = a.stamps + 4 * (size_t)(blockIdx.y * gridDim.x + blockIdx.x);
        o[0] = st_t0;
        o[1] = st_r0;
        o[2] = __builtin_amdgcn_s_memtime();
        o[3] = __builtin_amdgcn_s_memrealtime();
    }
#endif
}

template <class OP>
__global__ __launch_bounds__(OP::kNW * 64) void filter_kernel(const FilterArgs a)
{
    filter_main<OP>(a);
}
// the split-bf16 operators (OpSplitT) under a kernel name of their own
template <class OP>
__global__ __launch_bounds__(OP::kNW * 64) void filter_split_kernel(const FilterArgs a)
{
    filter_main<OP>(a);
}

// the lazy split operators (OpLazySplitT)
template <class OP>
__global__ __launch_bounds__(OP::kNW * 64) void filter_lazy_kernel(const FilterArgs a)
{
    filter_main<OP>(a);
}

// the lazy schedule on 16x16x32 tiles (OpLazySplit16)
// (a search of an index that keeps the int8 pre-pass's operands enqueues this kernel AND filter_i8pre_kernel; both read
//  the selection words K2 left and the one they do not name returns at once: no host read, the search stays asynchronous)
template <class OP>
__global__ __launch_bounds__(OP::kNW * 64) void filter_lazy16_kernel(const FilterArgs a)
{
    if (a.pre.q8 && i8pre_selected(a.scal->i8_cmax_bits, a.scal->i8_odd_count, a.pre.m, a.pre.force != 0)) return;
    filter_main<OP>(a);
}
// fp16 points (OpF16T)
template <class OP>
__global__ __launch_bounds__(OP::kNW * 64) void filter_f16_kernel(const FilterArgs a)
{
    filter_main<OP>(a);
}
// int8 points (OpI8)
template <class OP>
__global__ __launch_bounds__(OP::kNW * 64) void filter_i8_kernel(const FilterArgs a)
{
    filter_main<OP>(a);
}
// the int8 pre-pass of the lazy schedule (OpI8Pre)
template <class OP>
__global__ __launch_bounds__(OP::kNW * 64) void filter_i8pre_kernel(const FilterArgs a)
{
    if (!i8pre_selected(a.scal->i8_cmax_bits, a.scal->i8_odd_count, a.pre.m, a.pre.force != 0)) return;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) const_cast<DevScalars *>(a.scal)->i8_ran = 1;
    filter_main<OP>(a);
}
// (the 32x32x16 lazy kernel stays in every build, launched or not: the ISA checks of the two read one compilation)
template __global__ void filter_lazy_kernel<OpLazySplit>(const FilterArgs a);
template __global__ void filter_lazy16_kernel<OpLazySplit16>(const FilterArgs a);

// ---- self-test: one 32x32 tile through the same MFMA k-order as the filter --------
// out[i][j] = accumulate over the image's k order of a[i][.] * b[j][.] seeded with c0[i];
// a, b are [32][kt] fp32 (bf16 mode: values must be bf16-representable).  Lets the tests
// check the hardware against host arithmetic — the error model behind tau.
__global__ __launch_bounds__(64) void mfma_selftest_kernel(int kt, int mode, const float *__restrict__ a,
                                                           const float *__restrict__ b,
                                                           const float *__restrict__ c0,
                                                           float *__restrict__ out)
{
    const int lane = threadIdx.x, h = lane >> 5, i = lane & 31;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = c0[(r & 3) + 8 * (r >> 2) + 4 * h];
    if (mode == ST_F32) {
        for (int s = 0; s < kt / 2; ++s) {
            const int kk = 8 * (s >> 2) + 4 * h + (s & 3);   // same k permutation as the image
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i * kt + kk], b[i * kt + kk], acc, 0, 0, 0);
        }
    } else if (mode == ST_BF16) {
        for (int s = 0; s < kt / 16; ++s) {
            bf16x8 av, bv;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                av[e] = (__bf16)a[i * kt + 16 * s + 8 * h + e];
                bv[e] = (__bf16)b[i * kt + 16 * s + 8 * h + e];
            }
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc, 0, 0, 0);
        }
    } else if (mode == ST_SPLIT) {
        // the split chain of OpSplitT: v = h + l, h = rn_bf16(v), l = rn_bf16(v - h); per 16-dim k-step (same lane
        // order as ST_BF16) ah.bh, ah.bl (the ref hi fragment's two MFMAs), then al.bh (the lo fragment's)
        for (int s = 0; s < kt / 16; ++s) {
            bf16x8 ah, al, bh, bl;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float av = a[i * kt + 16 * s + 8 * h + e], bv = b[i * kt + 16 * s + 8 * h + e];
                ah[e] = (__bf16)av;
                al[e] = (__bf16)__fsub_rn(av, (float)ah[e]);
                bh[e] = (__bf16)bv;
                bl[e] = (__bf16)__fsub_rn(bv, (float)bh[e]);
            }
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
        }
    } else if (mode == ST_LAZY) {
        // the lazy order of OpLazySplitT: the kt / 16 hi-hi MFMAs (partial result to out + 1024), then per k-step al.bh
        // (ref hi x query lo) and ah.bl on the same accumulator.  (a = query rows, b = ref rows as above.)
        for (int pass = 0; pass < 2; ++pass) {
            for (int s = 0; s < kt / 16; ++s) {
                bf16x8 ah, al, bh, bl;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float av = a[i * kt + 16 * s + 8 * h + e], bv = b[i * kt + 16 * s + 8 * h + e];
                    ah[e] = (__bf16)av;
                    al[e] = (__bf16)__fsub_rn(av, (float)ah[e]);
                    bh[e] = (__bf16)bv;
                    bl[e] = (__bf16)__fsub_rn(bv, (float)bh[e]);
                }
                if (pass == 0) {
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
                } else {
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
                }
            }
            if (pass == 0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) out[1024 + ((r & 3) + 8 * (r >> 2) + 4 * h) * 32 + i] = acc[r];
            }
        }
    } else if (mode == ST_I8) {
        // mode 2's four 16x16 tiles and lane mapping on v_mfma_i32_16x16x64_i8 (OpI8 and K2's int8 image): lane l holds dims
        // 64 ks + 16 (l >> 4) .. + 15 of row l & 15, byte j of the four operand registers = dim j of the sixteen; operands
        // cast to int8, the i32 accumulator seeded with c0 and returned as fp32
        const int c = lane & 15, g = lane >> 4;
        for (int rt = 0; rt < 2; ++rt)
            for (int qt = 0; qt < 2; ++qt) {
                i32x4 t;
#pragma unroll
                for (int e = 0; e < 4; ++e) t[e] = (int)c0[16 * rt + 4 * g + e];
                for (int ks = 0; ks < kt / 64; ++ks) {
                    i32x4 av, bv;
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        unsigned aw = 0, bw = 0;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            aw |= (unsigned)(unsigned char)(int8_t)(int)a[(16 * rt + c) * kt + 64 * ks + 16 * g + 4 * w + j] << (8 * j);
                            bw |= (unsigned)(unsigned char)(int8_t)(int)b[(16 * qt + c) * kt + 64 * ks + 16 * g + 4 * w + j] << (8 * j);
                        }
                        av[w] = (int)aw;
                        bv[w] = (int)bw;
                    }
                    t = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, bv, t, 0, 0, 0);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) out[(16 * rt + 4 * g + e) * 32 + 16 * qt + c] = (float)t[e];
            }
        return;
    } else if (mode == ST_F16) {
        // mode 2's four 16x16 tiles and lane mapping on v_mfma_f32_16x16x32_f16, operands cast to binary16 (OpF16T)
        const int c = lane & 15, g = lane >> 4;
        for (int rt = 0; rt < 2; ++rt)
            for (int qt = 0; qt < 2; ++qt) {
                f32x4 t;
#pragma unroll
                for (int e = 0; e < 4; ++e) t[e] = c0[16 * rt + 4 * g + e];
                for (int ks = 0; ks < kt / 32; ++ks) {
                    f16x8 av, bv;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        av[e] = (_Float16)a[(16 * rt + c) * kt + 32 * ks + 8 * g + e];
                        bv[e] = (_Float16)b[(16 * qt + c) * kt + 32 * ks + 8 * g + e];
                    }
                    t = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, bv, t, 0, 0, 0);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) out[(16 * rt + 4 * g + e) * 32 + 16 * qt + c] = t[e];
            }
        return;
    } else {
        // ST_BF16_T16: the same 32x32 product as four 16x16 tiles of v_mfma_f32_16x16x32_bf16, with
        // the operand / result lane mapping the filter's OpBF16T and K2's order 1 image assume
        const int c = lane & 15, g = lane >> 4;
        for (int rt = 0; rt < 2; ++rt)
            for (int qt = 0; qt < 2; ++qt) {
                f32x4 t;
#pragma unroll
                for (int e = 0; e < 4; ++e) t[e] = c0[16 * rt + 4 * g + e];
                for (int ks = 0; ks < kt / 32; ++ks) {
                    bf16x8 av, bv;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        av[e] = (__bf16)a[(16 * rt + c) * kt + 32 * ks + 8 * g + e];
                        bv[e] = (__bf16)b[(16 * qt + c) * kt + 32 * ks + 8 * g + e];
                    }
                    t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, t, 0, 0, 0);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) out[(16 * rt + 4 * g + e) * 32 + 16 * qt + c] = t[e];
            }
        return;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) out[((r & 3) + 8 * (r >> 2) + 4 * h) * 32 + i] = acc[r];
}

// ---- self-test of OpLazySplit16's operands and chain: one wave, 32 refs x 64 queries at KT = 128 -------------------
// q [64][128], r [32][128] fp32, c0 [32]: the wave first writes the split images in the order K2 writes them (32x32x16
// operand order; refs: hi and lo regions as form 3, queries: qh | ql interleaved per 16-dim step as form 2), then takes
// its 16x16x32 operands out of them through lazy16_gather and runs the kernel's chain: the four hi-hi MFMAs seeded with
// c0 (-> out_hh), then rh x ql and rl x qh per k-step on the same accumulator (-> out).  Both [ref][query].
__global__ __launch_bounds__(64) void mfma_lazy16_selftest_kernel(const float *__restrict__ q, const float *__restrict__ r,
                                                                  const float *__restrict__ c0, float *__restrict__ out,
                                                                  float *__restrict__ out_hh)
{
    constexpr int KT = 128;
    __shared__ bf16x8 rimg[2][8 * 64];        // [hi | lo][fragment s][lane]
    __shared__ bf16x8 qimg[2][16 * 64];       // [query block][2 s + part][lane]
    const int lane = threadIdx.x, hl = lane >> 5, p = lane & 31;
    auto split8 = [](const float *v, bf16x8 &h, bf16x8 &l) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            h[e] = (__bf16)v[e];
            l[e] = (__bf16)__fsub_rn(v[e], (float)h[e]);
        }
    };
    for (int s = 0; s < KT / 16; ++s) {       // lane 32 hl + p of fragment s: dims 16 s + 8 hl .. + 7 of point p
        split8(r + p * KT + 16 * s + 8 * hl, rimg[0][s * 64 + lane], rimg[1][s * 64 + lane]);
        for (int qb = 0; qb < 2; ++qb)
            split8(q + (32 * qb + p) * KT + 16 * s + 8 * hl, qimg[qb][(2 * s) * 64 + lane], qimg[qb][(2 * s + 1) * 64 + lane]);
    }
    __syncthreads();
    const int g = lane >> 4, i = lane & 15;
    for (int rt = 0; rt < 2; ++rt)
        for (int st = 0; st < 4; ++st) {
            f32x4 t;
#pragma unroll
            for (int e = 0; e < 4; ++e) t[e] = c0[16 * rt + 4 * g + e];
            for (int ks = 0; ks < KT / 32; ++ks)
                t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(rimg[0][lazy16_gather(lane, rt, ks)],
                                                            qimg[st >> 1][lazy16_gather(lane, st & 1, ks, 2, 0)], t, 0, 0, 0);
#pragma unroll
            for (int e = 0; e < 4; ++e) out_hh[(16 * rt + 4 * g + e) * 64 + 16 * st + i] = t[e];
            for (int ks = 0; ks < KT / 32; ++ks) {
                t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(rimg[0][lazy16_gather(lane, rt, ks)],
                                                            qimg[st >> 1][lazy16_gather(lane, st & 1, ks, 2, 1)], t, 0, 0, 0);
                t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(rimg[1][lazy16_gather(lane, rt, ks)],
                                                            qimg[st >> 1][lazy16_gather(lane, st & 1, ks, 2, 0)], t, 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) out[(16 * rt + 4 * g + e) * 64 + 16 * st + i] = t[e];
        }
}

int launch_mfma_lazy16_selftest(const float *q, const float *r, const float *c0, float *out, float *out_hh, hipStream_t st)
{
    hipLaunchKernelGGL(mfma_lazy16_selftest_kernel, dim3(1), dim3(64), 0, st, q, r, c0, out, out_hh);
    NNS_HIP(hipGetLastError());
    return NNS_OK;
}

// ---- self-test of OpI8Pre's operands and chain: one wave, 32 refs x 64 queries at KT = 128 --------------------------------
// q [64][128], r [32][128] int8, seeds [32] i32: the wave writes the two int8 images as K2 writes them (fragment 2 t + ks:
// lane l holds dims 64 ks + 16 (l >> 4) .. + 15 of point 16 t + (l & 15); the refs NEGATED), then runs the kernel's chain
// through the operator's own MFMAs: the seed MFMA of k-step 0 with the lane's four seeds as srcC, then k-step 1.
// out [ref][query] = seeds[ref] - q.r, exact integers.
__global__ __launch_bounds__(64) void mfma_i8pre_selftest_kernel(const int8_t *__restrict__ q, const int8_t *__restrict__ r,
                                                                 const int *__restrict__ seeds, int *__restrict__ out)
{
    __shared__ uint4 rimg[4 * 64], qimg[8 * 64];   // [fragment 2 t + ks][lane]
    const int lane = threadIdx.x, g = lane >> 4, i = lane & 15;
    auto pack = [&](const int8_t *row, bool neg) {
        unsigned w[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            w[e] = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int v = row[4 * e + b];
                w[e] |= (unsigned)(unsigned char)(int8_t)(neg ? -v : v) << (8 * b);
            }
        }
        return make_uint4(w[0], w[1], w[2], w[3]);
    };
    for (int f = 0; f < 8; ++f) {
        const int t = f >> 1, ks = f & 1;
        qimg[f * 64 + lane] = pack(q + (16 * t + i) * 128 + 64 * ks + 16 * g, false);
        if (f < 4) rimg[f * 64 + lane] = pack(r + (16 * t + i) * 128 + 64 * ks + 16 * g, true);
    }
    __syncthreads();
    for (int rt = 0; rt < 2; ++rt)
        for (int st = 0; st < 4; ++st) {
            const int4 sd = *reinterpret_cast<const int4 *>(seeds + 16 * rt + 4 * g);
            const f32x4 c = __builtin_bit_cast(f32x4, i32x4{sd.x, sd.y, sd.z, sd.w});
            f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
            OpI8Pre::mma16_seed(__builtin_bit_cast(float4, rimg[(2 * rt) * 64 + lane]), __builtin_bit_cast(float4, qimg[(2 * st) * 64 + lane]), acc, c);
            OpI8Pre::mma16(__builtin_bit_cast(float4, rimg[(2 * rt + 1) * 64 + lane]), __builtin_bit_cast(float4, qimg[(2 * st + 1) * 64 + lane]), acc);
            const i32x4 o = __builtin_bit_cast(i32x4, acc);
#pragma unroll
            for (int e = 0; e < 4; ++e) out[(16 * rt + 4 * g + e) * 64 + 16 * st + i] = o[e];
        }
}

int launch_mfma_i8pre_selftest(const int8_t *q, const int8_t *r, const int *seeds, int *out, hipStream_t st)
{
    hipLaunchKernelGGL(mfma_i8pre_selftest_kernel, dim3(1), dim3(64), 0, st, q, r, seeds, out);
    NNS_HIP(hipGetLastError());
    return NNS_OK;
}

// self-test of share_min: out[l] = the value lane l would adopt from in[0..63]
__global__ __launch_bounds__(64) void lane_share_selftest_kernel(int t16, const float *__restrict__ in, float *__restrict__ out)
{
    const float t = in[threadIdx.x];
    out[threadIdx.x] = t16 ? share_min<true>(t) : share_min<false>(t);
}

int launch_lane_share_selftest(int t16, const float *in, float *out, hipStream_t st)
{
    hipLaunchKernelGGL(lane_share_selftest_kernel, dim3(1), dim3(64), 0, st, t16, in, out);
    NNS_HIP(hipGetLastError());
    return NNS_OK;
}

int launch_mfma_selftest(int kt, int mode, const float *a, const float *b, const float *c0, float *out,
                         hipStream_t st)
{
    hipLaunchKernelGGL(mfma_selftest_kernel, dim3(1), dim3(64), 0, st, kt, mode, a, b, c0, out);
    NNS_HIP(hipGetLastError());
    return NNS_OK;
}

// ---- planning + launch ---------------------------------------------------------------
// streams of at most this many 32-ref tiles per workgroup run with shared lane thresholds
constexpr int64_t kShareThrMaxTiles = 2048;
#ifndef NNS_F_TILEREC_MAX
#define NNS_F_TILEREC_MAX 2048
#endif
constexpr int64_t kTileRecMaxTiles = NNS_F_TILEREC_MAX;

// Depths at which fp32 points take the split-bf16 operands (OpSplitT) unless NNS_FILTER_F32 is given: all five, each
// won a same-device A/B at 65536 x 1048576 (filter 3.3x at KT 16, 3.4x at 32, 3.7x at 64 and 128, 3.5x at 256, keys
// bit-equal: profiles/split_ab_depths.jsonl)
constexpr bool split_depth(int kt)
{
    return kt == 16 || kt == 32 || kt == 64 || kt == 128 || kt == 256;
}

// Depths at which the split operands run the lazy schedule (OpLazySplitT) unless NNS_FILTER_SPLIT_EAGER is given: KT = 128
// (C3: profiles/lazy_ab_depths.jsonl).  The other depths keep the eager kernels until a same-device A/B shows a win.
constexpr bool lazy_depth(int kt)
{
    return kt == 128;
}

// The MFMA shape of the lazy kernel at KT = 128: 1 = OpLazySplit16 (16x16x32), 0 = OpLazySplit (32x32x16).  Both run the same plan
// on the same image and fill the same lists (A/B builds: tools/build_variant.sh <name> -DNNS_F_LAZY_T16=0).
#ifndef NNS_F_LAZY_T16
#define NNS_F_LAZY_T16 1
#endif
using LazyOp128 = std::conditional_t<NNS_F_LAZY_T16 != 0, OpLazySplit16, OpLazySplit>;
static_assert(OpLazySplit16::kQB * OpLazySplit16::kNW * 32 == 512 && OpLazySplit::kQB * OpLazySplit::kNW * 32 == 512,
              "both lazy operators: 512 queries per workgroup (filter_plan sizes the query groups from the eager twin)");
int filter_lazy_tile()
{
    return LazyOp128::kTile16 ? 16 : 32;
}

// The one (form, depth)-to-operator table: f(OP{}) for the operator that runs geometry g.  The depths listed here are
// the forms' ladders (kFilterForms).  (The cases stand in the order the operators' kernels are laid out in the code object.)
template <class F>
static int with_filter_op(const FilterGeom &g, F &&f)
{
    switch (g.form) {
    case FORM_I8:
        if (g.kt == 256) return f(OpI8{});
        break;
    case FORM_F16:
        switch (g.kt) {
        case 128: return f(OpF16K128{});
        case 256: return f(OpF16{});
        }
        break;
    case FORM_BF16:
    case FORM_MIXED:
        switch (g.kt) {
        case 128: return f(OpBF16K128{});   // 4 k-steps per 16-ref tile, 4 blocks per slot
        case 256: return f(OpBF16{});
        case 384: return f(OpBF16K384{});   // four 24-step blocks over three ring slots
        case 512: return f(OpBF16K512T{});
        case 640: return f(OpBF16K640{});   // four 40-step blocks over five ring slots
        case 768: return f(OpBF16K768{});   // two 48-step blocks over three ring slots
        case 1024: return f(OpBF16K1024{}); // K-split accumulation over two ring slots per block
        }
        break;
    case FORM_SPLIT:
        if (g.lazy) {
            if (g.kt == 128) return f(LazyOp128{});
            break;
        }
        switch (g.kt) {
        case 16: return f(OpSplitK16{});
        case 32: return f(OpSplitK32{});
        case 64: return f(OpSplitK64{});
        case 128: return f(OpSplit{});
        case 256: return f(OpSplitK256{});
        }
        break;
    case FORM_F32:
        switch (g.kt) {
        case 16: return f(OpF32K16{});      // 2 fragment steps per block, 16 blocks per slot
        case 32: return f(OpF32K32{});      // 4 fragment steps per block, 8 blocks per slot
        case 64: return f(OpF32K64{});      // 8 steps per block, 4 blocks per slot
        case 128: return f(OpF32{});
        case 256: return f(OpF32K256{});    // 32 fragment steps per block, 1 block per slot
        }
        break;
    }
    set_error("MFMA filter: no operator for kt = %d (bf16 %d, split %d, lazy %d)", g.kt,
              (unsigned)g.form < FORM_COUNT ? kFilterForms[g.form].bf16 : 0, g.form == FORM_SPLIT, g.lazy);
    return NNS_ERR_UNSUPPORTED;
}

int filter_plan(const FilterRequest &rq, FilterGeom *g)
{
    const int k = rq.k, m = rq.m, n = rq.n;
    const bool per_ref = rq.per_ref, split_eager = rq.split_eager;
    const int form = (unsigned)rq.form < FORM_COUNT ? rq.form : FORM_BF16;   // (FORM_NONE: no caller plans a type without a filter)
    const FilterForm &ff = kFilterForms[form];
    int kt = 0;
    for (int i = 0; i < 8 && ff.ladder[i] && !kt; ++i)
        if (k <= ff.ladder[i]) kt = ff.ladder[i];
    if (!kt) {
        if (form == FORM_F16 || form == FORM_I8)   // (the two forms whose refusal names the points)
            set_error("MFMA filter: k = %d exceeds the deepest tile of %s points (256)", k, ff.name);
        else
            set_error("MFMA filter: k = %d exceeds the deepest tile (fp32 operands: 256, bf16 operands: 1024)", k);
        return NNS_ERR_UNSUPPORTED;
    }
    g->dtype = (unsigned)rq.dtype < DT_COUNT ? rq.dtype : DT_BF16;   // (point_type's rule for a code the ABI does not define)
    // (the split form shares every geometry field below with the fp32 one: same blocks, slots and queries per wave)
    g->form = form == FORM_SPLIT && !split_depth(kt) ? FORM_F32 : form;
    g->kt = kt;
    // (the schedule is chosen at the end, from the stream length that the query groups fix: the lazy operator has its
    //  eager twin's tiles and workgroup)
    static_assert(OpLazySplit::kQB * OpLazySplit::kNW == OpSplit::kQB * OpSplit::kNW, "lazy and eager split: same query groups");
    g->lazy = g->lazy_img = 0;
    // the operator's tile and workgroup (read with lazy = 0: the eager operator, whose blocks the image is made of)
    NNS_TRY(with_filter_op(*g, [g](auto op) {
        using OP = decltype(op);
        // (K7m's flag kernel, range_mfma.hip, takes its workgroup and ring slot from these two constants)
        if constexpr (OP::kSplit && !OP::kLazy)
            static_assert(OP::kNW == kSplitWaves && OP::kSlotSteps == kSplitSlotSteps, "the eager split operators' workgroup and slot");
        // (and its bf16 flag kernel at KT = 128 / 256: the same ring, OpBF16K128 / OpBF16's blocks and query groups)
        if constexpr (OP::kTile16 && !OP::kSplit && !OP::kLazy && (OP::kSPB == 8 || OP::kSPB == 16))
            static_assert(OP::kNW == kSplitWaves && OP::kSlotSteps == kSplitSlotSteps && OP::kQB == kFlag16QB,
                          "the 16x16x32 bf16 operators' workgroup, slot and query blocks per wave");
        g->lpq = OP::kLPQ;
        g->spb = OP::kSPB;
        g->qb = OP::kQB;
        g->waves = OP::kNW;
        g->qw = 32 * OP::kQB * OP::kNW;
        return (int)NNS_OK;
    }));
    const int qw = g->qw;
    g->m_pad = divup(m, qw) * qw;
    // the ring of 32-step slots (8 fp32 / 16 bf16 dims per step): the refs are padded to whole super-periods; slot_pts,
    // which only sizes paddings from here on, is rounded up where a slot holds a fraction of a block (768-deep: 21.33 refs)
    const RingGeom ring = ring_geom(g->spb);
    const int slots_per_block = ring.slots, pad_pts = ring.slot_refs;
    const int slot_pts = divup(pad_pts, slots_per_block);
    g->n_pad = divup(n, pad_pts) * pad_pts;
    g->total_slots = g->n_pad / pad_pts * slots_per_block;
    g->qgroups = g->m_pad / qw;
    // ref-range splits: within 2 GiB of candidate lists (512 B per lane-list: 1 or 2 KiB per query per split)
    const int64_t list_cap = (int64_t)2 << 30;
    const int splits = ring_pass_splits(g->qgroups, g->total_slots, list_cap / ((int64_t)g->m_pad * g->lpq * 512));
    g->slots_per_split = divup(divup(g->total_slots, splits), slots_per_block) * slots_per_block;   // whole blocks
    g->splits = divup(g->total_slots, g->slots_per_split);
    g->slot_pts = slot_pts;
    // short streams (every tile of a stream of T tiles is slow until ~64 tiles in): share thresholds among a query's
    // lanes, and record tiles instead of single scores; long streams (C3: 16384 tiles, C5: 8192) keep private
    // thresholds and per-score records.  Tile records need K5's one-wave-per-query form (splits >= 4: a tile's rows
    // are evaluated by 16 lanes side by side).
    const int64_t stream_tiles = (int64_t)g->slots_per_split / slots_per_block * (pad_pts / 32);
    // (fp32 points through bf16 operands: the rounding term makes tau ~2^-6 |x'||y'|, thousands of refs lie within it
    //  of the running minimum, and private thresholds fill the 64-entry rings — 5 504 of 65 536 queries overflowed into
    //  the exact scan at k = 1024 — so their lanes always share, whatever the stream length)
    g->share_thr = (stream_tiles <= kShareThrMaxTiles || g->form == FORM_MIXED) ? 1 : 0;
    // record forms: 0 per score (long streams), 1 per (lane, ref tile) behind the threshold test (short streams, 16 x 16
    // bf16 tiles: their epilogue has no vector slots to spare), 2 the lane's two best tiles, branch-free (short streams,
    // 32 x 32 tiles: every fp32 depth and the 768- / 1024-deep bf16-operand tiles)
    g->tile_rec = (stream_tiles <= kTileRecMaxTiles && g->splits >= 4 && !per_ref) ? (g->lpq == 4 ? 1 : 2) : 0;
    // The lazy schedule: an index of a lazy depth keeps its image in the lazy layout whatever the query count (the
    // layout is fixed when the index is built); a search runs the lazy kernel where its records are per score, and the
    // eager kernel — reading the same image — on the short-stream record forms, where nearly every tile refines anyway.
    g->lazy_img = (g->form == FORM_SPLIT && lazy_depth(kt) && !split_eager) ? 1 : 0;
    g->lazy = (g->lazy_img && g->tile_rec == 0) ? 1 : 0;
    return NNS_OK;
}

template <class OP>
static int launch_filter_t(const FilterGeom &g, const FilterArgs &args, hipStream_t st)
{
    auto kern = [] {   // (one kernel per operator: a plain conditional would instantiate both names)
        if constexpr (OP::kPre) return filter_i8pre_kernel<OP>;
        else if constexpr (OP::kI8) return filter_i8_kernel<OP>;
        else if constexpr (OP::kF16) return filter_f16_kernel<OP>;
        else if constexpr (OP::kLazy && OP::kTile16) return filter_lazy16_kernel<OP>;
        else if constexpr (OP::kLazy) return filter_lazy_kernel<OP>;
        else if constexpr (OP::kSplit) return filter_split_kernel<OP>;
        else return filter_kernel<OP>;
    }();
    // + 2 KiB per wave for the lanes' tau constants
    constexpr int lds_bytes = F_LDS_BYTES<OP> + OP::kNW * 2048;
    // > 64 KiB of dynamic LDS needs the opt-in, once per device
    static std::atomic<bool> attr_set[64];   // (two threads racing here both set it: harmless)
    int dev = 0;
    NNS_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64 || !attr_set[dev].load(std::memory_order_acquire)) {
        NNS_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
        if (dev >= 0 && dev < 64) attr_set[dev].store(true, std::memory_order_release);
    }
    hipLaunchKernelGGL(kern, dim3(g.qgroups, g.splits), dim3(OP::kNW * 64), lds_bytes, st, args);
    NNS_HIP(hipGetLastError());
    return NNS_OK;
}

int launch_filter(const FilterGeom &g, const void *qimg, const void *rimg, const float *rnorm,
                  const float *qnorm, const DevScalars *scal, CandEntry *lists, int *counts,
                  hipStream_t st, const FilterPreArgs *pre)
{
    FilterArgs a;
    a.pre = pre ? *pre : FilterPreArgs{};
    a.qimg = reinterpret_cast<const float4 *>(qimg);
    a.rimg = reinterpret_cast<const char *>(rimg);
    a.rimg_lo = g.lazy_img ? a.rimg + (size_t)g.n_pad * g.kt * 2 : nullptr;   // (split operands only)
    a.rnorm = rnorm;
    a.qnorm = qnorm;
    a.scal = scal;
    a.lists = lists;
    a.counts = counts;
    a.total_slots = g.total_slots;
    a.slots_per_split = g.slots_per_split;
    a.m_pad = g.m_pad;
    a.kt = g.kt;
    a.tau_mode = filter_tau_mode(g);
    a.share_thr = g.share_thr;   // (filter_plan)
    a.tile_rec = g.tile_rec;
#ifdef NNS_DIAG
    a.stamps = nullptr;
    const char *clk = getenv("NNS_FILTER_CLOCK");
    const size_t nwg = (size_t)g.qgroups * g.splits;
    if (clk && atoi(clk)) {
        NNS_HIP(hipMalloc(&a.stamps, (nwg * 4 + 8) * sizeof(unsigned long long)));
        NNS_HIP(hipMemsetAsync(a.stamps, 0, (nwg * 4 + 8) * sizeof(unsigned long long), st));
    }
#endif
    if (pre && !(g.lazy && g.kt == 128 && LazyOp128::kTile16)) {
        set_error("MFMA filter: the int8 pre-pass serves the lazy 16x16 kernel at kt = 128 (kt = %d, lazy %d)", g.kt, g.lazy);
        return NNS_ERR_UNSUPPORTED;
    }
    int rc = with_filter_op(g, [&](auto op) { return launch_filter_t<decltype(op)>(g, a, st); });
    // (diagnostic builds: the two launches share a.stamps — the kernel the rule does not name returns before it touches
    //  them, so the stamps and totals read below are the running kernel's alone)
    if (rc == NNS_OK && pre) rc = launch_filter_t<OpI8Pre>(g, a, st);
#ifdef NNS_DIAG
    if (a.stamps) {   // diagnostic: synchronous read-out, median clock over workgroups
        std::vector<unsigned long long> h(nwg * 4 + 8);
        NNS_HIP(hipStreamSynchronize(st));
        NNS_HIP(hipMemcpy(h.data(), a.stamps, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        std::vector<double> ghz, us;
        unsigned long long first = ~0ull, last = 0;
        for (size_t w = 0; w < nwg; ++w)
            if (h[4 * w + 3] > h[4 * w + 1]) {
                ghz.push_back((double)(h[4 * w + 2] - h[4 * w]) / (double)(h[4 * w + 3] - h[4 * w + 1]) * 0.1);
                us.push_back((double)(h[4 * w + 3] - h[4 * w + 1]) * 0.01);   // 100 MHz ticks
                first = std::min(first, h[4 * w + 1]);
                last = std::max(last, h[4 * w + 3]);
            }
        std::sort(ghz.begin(), ghz.end());
        std::sort(us.begin(), us.end());
        if (!ghz.empty())
            fprintf(stderr, "[nns] filter in-kernel clock: median %.3f GHz (min %.3f, max %.3f) over %zu workgroups; "
                            "workgroup main loop %.1f us median (%.1f .. %.1f), first start to last end %.1f us\n",
                    ghz[ghz.size() / 2], ghz.front(), ghz.back(), ghz.size(), us[us.size() / 2], us.front(), us.back(),
                    (double)(last - first) * 0.01);
        // (the total words behind the stamps: slow-path executions, retirements, ticks inside the slow path, ticks inside
        //  sync_slot, waves)
        const double nwaves = h[nwg * 4 + 4] ? (double)h[nwg * 4 + 4] : 1.0;
        fprintf(stderr, "[nns] filter slow path: %llu of %llu (tile, state) retirements (fp32 tiles only), %.0f memtime ticks each, share=%d, "
                        "%.0f memtime ticks per wave in the slot wait + barrier\n",
                h[nwg * 4], h[nwg * 4 + 1], h[nwg * 4] ? (double)h[nwg * 4 + 2] / (double)h[nwg * 4] : 0.0, a.share_thr,
                (double)h[nwg * 4 + 3] / nwaves);
        (void)hipFree(a.stamps);
    }
#endif
    return rc;
}

}  // namespace nns
