// finalize.hip — K5: turn the filter's candidate lists into V0's answer.
//
// Role in the reference: the second-stage reductions — the LDS tree of get_min_kernel
// (core.cu:105-119), V7's host re-rank over per-block candidates (core.cu:675-696) and
// V8/V9's host merge over per-GPU candidates (core.cu:832-852; wrong for m > 1, SURVEY
// F4).  Here the candidates are re-ranked with V0's own arithmetic on the device and the
// result is a packed (distance, index) key, so splits / shards / GPUs merge with a plain
// integer min and the outcome is V0's argmin bit for bit.
//
// The proof.  For query i let s_j = |y'_j|^2 - 2 x'_i.y'_j be the filter score of ref j
// (fp32 MFMA chain, or bf16 MFMA with fp32 accumulate), a = min_j s_j, X^2 = |x'_i|^2,
// Y^2 = max_j |y'_j|^2 (K2's norms), u = 2^-24, K the tile depth, g = gamma_{K+2}.  Then for
// every j
//     | s_j + |x'|^2 - D_j |  <=  e3 + e2,        D_j = ||q_i - r_j||^2 in real arithmetic
//       e3 = g (Y^2 + 2XY) + 2u Y^2    K-step FMA chain seeded with the rounded norm
//                                       (v_mfma_f32_32x32x2_f32 is a k-ordered fmaf chain;
//                                       tests check that on the hardware; the bf16 MFMA's
//                                       internal order is undocumented: 2u per add assumed
//                                       and checked against fp64 by the tests)
//       e2 = 2.5u (X + Y)^2            the single rounding of x' = fl(x-c), y' = fl(y-c)
//                                       (0 on the bf16 path: no centring)
// (split-bf16 operands of fp32 points, tau mode 3: e3 also carries the dropped lo x lo / rounding terms and an
//  absolute floor for subnormal operand parts and products — tau_consts, DESIGN.md "Exactness")
// and V0's own fp32 value d0_j (core.cu:38-43: k+1 roundings per term) satisfies
// |d0_j - D_j| <= g D_j.  Hence with
//     tau(a) = 2 (e3 + e2) + 2g/(1-g) (max(a + X^2, 0) + e3 + e2)
// any ref with s_j > a + tau(a) has d0_j strictly above d0 of the filter's best ref:
// V0's argmin lies in C_i = { j : s_j <= a + tau(a) }.  The filter appends every such j
// to a list (its running threshold is never below a + tau(a), see filter_mfma.hip); this
// kernel evaluates V0's exact distance for the members of C_i (1-2 refs typically) and
// keeps the lexicographic (distance, index) minimum == V0's result, ties included.
// Lists that overflowed, NaN/INF/huge inputs (K2's max-|value| word) or an empty list
// send the query to the exact scan over all refs (K1b) instead.
//
// fp32 evaluation.  tau above is real arithmetic; the kernels compute, in fp32 (u = 2^-24, every operation
// rounded to nearest, nothing contracted),
//     tau_fl(a) = fl(c0 + fl(c1 * max(fl(a + x2), 0)))        K5:     T5(a) = fl(a + tau_fl(a))
//                                                              filter: Tf(t) = fl(t + fl(1.002 * tau_fl(t)))
// with c0 = 1.001 (2 + c1)(e3 + e2) + er, c1 = 1.001 * 2g/(1-g), x2 >= X^2 (tau_consts, then rounded UP to fp32).
//  (i)  tau_fl(a) >= tau_c(a) (1 - 3u), tau_c = the same expression in real arithmetic: three roundings, each
//       relative and downward by at most u.
//  (ii) T5(a) >= a + tau_fl(a) - u |a + tau_fl(a)| >= a + tau_c(a) (1 - 4u) - u |a|: the rounding of the threshold
//       sum is relative to the SCORE's magnitude, |a| <= max(X^2, Y^2 + 2XY) + e3 <= (X + Y)^2 + e3, i.e. up to
//       tau / (2 (K + 2)) — 2.8 % of tau at K = 16.  The factors 1.001 do not cover that; er = 2u ((X+Y)^2 + e3 + e2)
//       does: tau_c(a) - tau(a) >= 0.001 tau(a) + er, 0.001 tau >= 4u tau_c, er >= u |a|  ==>  T5(a) >= a + tau(a).
//       So K5 keeps every member of C_i.  (tests/test_tau_model.py evaluates T5 in fp32 over a grid of depths, norms
//       and scores and holds it against a + tau(a) in extended precision, and asserts slack >= u (|a| + tau).)
//  (iii) every fp32 operation above is monotone non-decreasing in a, so t >= a ==> Tf(t) >= Tf(a), and
//       fl(1.002 tau_fl) >= tau_fl gives Tf(a) >= T5(a): a lane's threshold — the minimum of Tf over the tile minima
//       it has seen, all >= the query's final minimum a — never drops below T5(a); whatever K5 selects was recorded.
//
// The lazy split filter's B (split_lazy_bound; K5 does not need it).  The lazy kernel tests a tile's HI-HI scores
// s_hh (the accumulator after the kt/16 qh.rh MFMAs) against fl(thr + B) and finishes only flagged tiles with the cross
// MFMAs, on the same accumulator: s_3 = s_hh + (computed qh.rl + ql.rh).  With a = 2^-8, |h| <= (1+a)|v|,
// |l| <= a(1+a)|v| and v = -2y':
//     s_hh - s_3 <= |qh.rl + ql.rh|                       <= 2a (1+a)^2 sum |x'_t v_t| <= 2a (1+a)^2 2XY
//                 + the 2kt + 2kt/16 adds behind the partial, 2u each on |partial sums| <= Y^2 + (1 + 2^-5) 2XY
//                 + mode 3's absolute floor (parts, products, adds below 2^-126).
// fl(thr + B) is ONE rounding at the score's magnitude, as in (ii): |thr + B| <= (X + Y)^2 (1 + small), and B carries
// 2u ((X + Y)^2 + ...) for it, so fl(thr + B) >= thr + (the three terms above).  Hence a tile with min s_hh > fl(thr + B)
// has no s_3 <= thr, contributes nothing in the eager kernel either, and running minimum, thresholds and recorded set
// are the eager kernel's up to summation order (the mode-3 accumulation model is order-free).  B ~ 2^-6 XY: half of
// mode 2's margin, 2^7 times mode 3's tau — it only decides which tiles are refined, never what is recorded.
// (tests/test_lazy_split_cpu.py: the split emulated exactly, both sums in the lazy order, fl(thr + B) in fp32.)
#include "nns_internal.h"
#ifdef NNS_DIAG
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#endif

namespace nns {

__device__ __forceinline__ float load_f(const float *p, size_t i) { return p[i]; }
__device__ __forceinline__ float load_f(const uint16_t *p, size_t i)
{
    return __uint_as_float((unsigned)p[i] << 16);   // bf16 -> fp32 widening is exact
}
__device__ __forceinline__ float4 load_f4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ float4 load_f4(const uint16_t *p)
{
    const uint2 v = *reinterpret_cast<const uint2 *>(p);
    float4 o;
    o.x = __uint_as_float(v.x << 16);
    o.y = __uint_as_float(v.x & 0xFFFF0000u);
    o.z = __uint_as_float(v.y << 16);
    o.w = __uint_as_float(v.y & 0xFFFF0000u);
    return o;
}

__device__ __forceinline__ float load_f(const f16_t *p, size_t i) { return pt_ld1(p + i); }   // fp16 -> fp32: exact
__device__ __forceinline__ float4 load_f4(const f16_t *p) { return pt_ld4(p); }
__device__ __forceinline__ float load_f(const i8_t *p, size_t i) { return pt_ld1(p + i); }    // int8 -> fp32: exact
__device__ __forceinline__ float4 load_f4(const i8_t *p) { return pt_ld4(p); }
__device__ __forceinline__ float load_f(const u8_t *p, size_t i) { return pt_ld1(p + i); }    // uint8 -> fp32: exact
__device__ __forceinline__ float4 load_f4(const u8_t *p) { return pt_ld4(p); }

// V0's exact distance (core.cu:38-43), t ascending; 4 dims per load when aligned
template <typename T>
__device__ __forceinline__ float v0_distance(const T *qi, const T *rj, int k, bool vec)
{
    float sum = 0.0f;
    if (vec) {
        for (int t = 0; t < k; t += 4) {
            const float4 qv = load_f4(qi + t), rv = load_f4(rj + t);
            sum = v0_step(sum, qv.x, rv.x);
            sum = v0_step(sum, qv.y, rv.y);
            sum = v0_step(sum, qv.z, rv.z);
            sum = v0_step(sum, qv.w, rv.w);
        }
    } else {
        for (int t = 0; t < k; ++t) sum = v0_step(sum, load_f(qi, t), load_f(rj, t));
    }
    return sum;
}

// V0's exact distance of the compacted evaluation (16- / 8-byte aligned rows, k % 4 == 0): the same chain as
// v0_distance — v0_step over t = 0 .. k - 1 in that order — with the loads of the next 32 dims (8 float4 of each row)
// issued before the chain over the current 32 runs, so a lane keeps 16 loads in flight instead of 2.
template <typename T>
__device__ __forceinline__ float v0_distance_ahead(const T *qi, const T *rj, int k)
{
    constexpr int CH = 8;   // float4 per row and chunk
    float sum = 0.0f;
    const int kc = k & ~(4 * CH - 1);
    float4 qa[CH], ra[CH];
    if (kc) {
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            qa[u] = load_f4(qi + 4 * u);
            ra[u] = load_f4(rj + 4 * u);
        }
    }
    int t = 0;
    for (; t < kc; t += 4 * CH) {
        float4 qb[CH], rb[CH];
        const bool more = t + 4 * CH < kc;   // (wave-uniform)
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            qb[u] = more ? load_f4(qi + t + 4 * (CH + u)) : qa[u];
            rb[u] = more ? load_f4(rj + t + 4 * (CH + u)) : ra[u];
        }
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            sum = v0_step(sum, qa[u].x, ra[u].x);
            sum = v0_step(sum, qa[u].y, ra[u].y);
            sum = v0_step(sum, qa[u].z, ra[u].z);
            sum = v0_step(sum, qa[u].w, ra[u].w);
        }
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            qa[u] = qb[u];
            ra[u] = rb[u];
        }
    }
    for (; t < k; t += 4) {
        const float4 qv = load_f4(qi + t), rv = load_f4(rj + t);
        sum = v0_step(sum, qv.x, rv.x);
        sum = v0_step(sum, qv.y, rv.y);
        sum = v0_step(sum, qv.z, rv.z);
        sum = v0_step(sum, qv.w, rv.w);
    }
    return sum;
}

// K5's candidate queue: capacity in (query slot, ref) pairs of a wave.  A unit of uniform clouds holds about one
// candidate per query and a few near ties (32.6 per 32-query unit at C3): one 64-lane evaluation round; the queue is drained
// whenever the next walk step would not fit, so a unit with thousands of candidates (duplicated refs) is more rounds.
constexpr int kK5Queue = 128;       // power of two, >= 64 (one walk step appends up to 64)
constexpr int kK5WalkAhead = 8;     // entry loads of a list in flight per walk step

#ifdef NNS_DIAG
// diagnostic builds (tools/probe_k5.py): [unit][8] per wave — s_memtime ticks of pass 1, of pass 2 as a whole and of its
// evaluations, evaluation rounds, lanes active in them, s_memrealtime ticks (100 MHz) of the wave, candidates
#define K5_DIAG_PARAM , unsigned long long *__restrict__ diag
#define K5_DIAG_ARG , diag
__device__ __forceinline__ unsigned long long k5_stamp()
{
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#else
#define K5_DIAG_PARAM
#define K5_DIAG_ARG
#endif

// One wave (= one workgroup) per list UNIT (the 64 lane-lists the filter's wave wrote for 32 queries x 2 lanes or 16
// queries x 4 lanes): lane L walks list lane L, so every load of the [entry][lane] layout is a fully coalesced 512-B
// row and the lpq lists of a query are walked in parallel.  Three phases:
//   1. minimum: a = the smallest score over the query's lists (kK5WalkAhead guarded entry loads in flight per list),
//      combined across the lanes L ^ 32 (^ 16); an overflowed or empty list makes the query a fallback.
//   2. compaction: the lists are walked again (L2 hits); a lane whose entry is within the threshold appends
//      (query slot, ref) to the wave's queue in LDS at the running count + lanes_below(ballot).  Nothing is evaluated
//      here: a candidate sits near the end of one of a query's lists, at a different entry position in every lane, and
//      evaluating inside the walk ran the 2 x 32 dependent row loads and V0's chain once per such position with one to
//      three lanes active.
//   3. evaluation: lane t takes queue entry t — V0's distance of its (query, ref), make_key — and merges into its
//      query's slot with a 64-bit LDS minimum, counting the candidates there: every lane of a round is live.
// The candidate set, the per-candidate arithmetic and the minimum over packed keys are those of the one-lane-per-list
// evaluation, so keys, fallbacks and multi-candidate queries are the same for every input.
template <typename T>
__global__ __launch_bounds__(64) void finalize_kernel(
    int kt, int tau_mode, int lpq, int m_pad, int splits, int k, int m, int n, const T *__restrict__ q,
    const T *__restrict__ r, const CandEntry *__restrict__ lists, const int *__restrict__ counts,
    const float *__restrict__ qnorm, DevScalars *__restrict__ scal, int64_t index_base,
    nns_key *__restrict__ keys, int *__restrict__ amb_list, int *__restrict__ multi_list K5_DIAG_PARAM)
{
    __shared__ uint2 queue[kK5Queue];           // (query slot within the unit, ref)
    __shared__ unsigned long long sbest[32];    // per query slot: the minimum key ...
    __shared__ int sncand[32];                  // ... and the number of candidates evaluated
    const int ush = lpq == 4 ? 4 : 5, qmask = (1 << ush) - 1;   // queries per list unit: 16 or 32
    const int lane = threadIdx.x;
    const int unit = blockIdx.x;
    const int units = m_pad >> ush;
    const int i = (unit << ush) + (lane & qmask);               // this lane's query
    const bool live = i < m;
#ifdef NNS_DIAG
    const unsigned long long d_r0 = __builtin_amdgcn_s_memrealtime();
    const unsigned long long d_t0 = k5_stamp();
    unsigned long long d_eval = 0;
    unsigned d_rounds = 0, d_active = 0;
#endif
    if (lane < 32) {
        sbest[lane] = NNS_KEY_NONE;
        sncand[lane] = 0;
    }

    // (mode 4, fp16 points: a ref beyond kF16RefMax has no finite scaled operand — the host latch's twin)
    bool fallback = scal->q_maxabs_bits >= kHugeBits || refs_void(scal->r_maxabs_bits, tau_mode == TAU_F16);
    float a = __builtin_inff();
    int over = 0;
    if (!fallback && live) {
        for (int s = 0; s < splits; ++s) {
            const size_t lblk = (size_t)s * units + unit;
            const int cw = counts[lblk * 64 + lane];
            if (cw & kCandOverflow) over = 1;
            const int c = (cw & kCandCountMask) < kCandCap ? (cw & kCandCountMask) : kCandCap;
            const CandEntry *l = lists + lblk * (kCandCap * 64) + lane;
            for (int e0 = 0; e0 < c; e0 += kK5WalkAhead) {
                float sc[kK5WalkAhead];
#pragma unroll
                for (int u = 0; u < kK5WalkAhead; ++u) sc[u] = e0 + u < c ? l[(e0 + u) * 64].s : __builtin_inff();
#pragma unroll
                for (int u = 0; u < kK5WalkAhead; ++u) a = fminf(a, sc[u]);
            }
        }
    }
    // combine the query's lpq lists: lanes that differ in the bits above the query index
    for (int off = 32; off >= (1 << ush); off >>= 1) {
        a = fminf(a, __shfl_xor(a, off, 64));
        over |= __shfl_xor(over, off, 64);
    }
    if (over || !(a < __builtin_inff())) fallback = true;
#ifdef NNS_DIAG
    const unsigned long long d_t1 = k5_stamp();
#endif

    const bool vec = (k & 3) == 0 && (((uintptr_t)q | (uintptr_t)r) & (4 * sizeof(T) - 1)) == 0;
    int qn = 0;   // entries in the queue (wave-uniform)
    // evaluation of the queue's qn entries, 64 per round (wave-uniform call sites; the barriers are one wave's)
    auto drain = [&]() {
#ifdef NNS_DIAG
        const unsigned long long d_e0 = k5_stamp();
#endif
        __syncthreads();   // the appends are visible
        for (int t0 = 0; t0 < qn; t0 += 64) {
            const int t = t0 + lane;
            if (t < qn) {
                const uint2 cand = queue[t];
                const T *qi = q + (size_t)((unit << ush) + (int)cand.x) * k, *rj = r + (size_t)cand.y * k;
                const float sum = vec ? v0_distance_ahead(qi, rj, k) : v0_distance(qi, rj, k, false);
                const nns_key key = make_key(sum, index_base + (int)cand.y);
                atomicMin(&sbest[cand.x], (unsigned long long)key);
                atomicAdd(&sncand[cand.x], 1);
            }
#ifdef NNS_DIAG
            ++d_rounds;
            d_active += qn - t0 < 64 ? qn - t0 : 64;
#endif
        }
        __syncthreads();   // the queue's entries are read before it is refilled
        qn = 0;
#ifdef NNS_DIAG
        d_eval += k5_stamp() - d_e0;
#endif
    };

    float thr = 0.0f;
    const bool walks = !fallback && live;
    if (walks) {
        const TauConsts tc = tau_consts(kt, qnorm[i], __uint_as_float(scal->ymax2_bits), tau_mode);
        thr = a + tau_of(tc, a);
    }
    for (int s = 0; s < splits; ++s) {
        const size_t lblk = (size_t)s * units + unit;
        int c = 0;
        if (walks) {
            const int cw = counts[lblk * 64 + lane] & kCandCountMask;
            c = cw < kCandCap ? cw : kCandCap;
        }
        const CandEntry *l = lists + lblk * (kCandCap * 64) + lane;
        int cmax = c;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int o = __shfl_xor(cmax, off, 64);
            cmax = o > cmax ? o : cmax;
        }
        cmax = __builtin_amdgcn_readfirstlane(cmax);
        for (int e0 = 0; e0 < cmax; e0 += kK5WalkAhead) {
            CandEntry ce[kK5WalkAhead];
#pragma unroll
            for (int u = 0; u < kK5WalkAhead; ++u) {
                ce[u].s = __builtin_inff();
                ce[u].j = n;
                if (e0 + u < c) ce[u] = l[(e0 + u) * 64];
            }
            // (rolled: one copy of the evaluation; the entry of step u is selected out of the registers)
#pragma unroll 1
            for (int u = 0; u < kK5WalkAhead && e0 + u < cmax; ++u) {
                CandEntry x = ce[0];
#pragma unroll
                for (int v = 1; v < kK5WalkAhead; ++v)
                    if (u == v) x = ce[v];
                const bool hit = e0 + u < c && x.s <= thr && x.j < n;
                const unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
                if (mask == 0) continue;   // (wave-uniform, as is the drain)
                const int add = __builtin_popcountll(mask);
                if (qn + add > kK5Queue) drain();
                if (hit) queue[qn + lanes_below(mask)] = make_uint2((unsigned)(lane & qmask), (unsigned)x.j);
                qn += add;
            }
        }
    }
    drain();
#ifdef NNS_DIAG
    const unsigned long long d_t2 = k5_stamp();
#endif

    if (live && lane <= qmask) {   // one lane per query writes
        const nns_key best = sbest[lane];
        const int ncand = sncand[lane];
        // every candidate NaN/INF cannot happen with bounded inputs; be safe anyway
        if (best == NNS_KEY_NONE) fallback = true;
        keys[i] = fallback ? (nns_key)NNS_KEY_NONE : best;
        if (fallback) {
            const int pos = atomicAdd(&scal->amb_count, 1);
            amb_list[pos] = i;
        } else if (ncand > 1) {    // decided by the exact re-rank of several candidates (rare)
            const int pos = atomicAdd(&scal->multi_count, 1);
            multi_list[pos] = i;
        }
    }
#ifdef NNS_DIAG
    if (diag && lane == 0) {
        unsigned long long *o = diag + 8 * (size_t)unit;
        o[0] = d_t1 - d_t0;
        o[1] = d_t2 - d_t1;
        o[2] = d_eval;
        o[3] = d_rounds;
        o[4] = d_active;
        o[5] = __builtin_amdgcn_s_memrealtime() - d_r0;
    }
#endif
}

#if defined(NNS_DIAG) && defined(NNS_K5_SPARSE)
// Diagnostic builds only (-DNNS_DIAG -DNNS_K5_SPARSE): the schedule finalize_kernel replaced — lane L evaluates its
// candidates inside its own list walk — with the stamps of the diagnostic buffer, to measure what the compaction buys.
template <typename T>
__global__ __launch_bounds__(64) void finalize_sparse_kernel(
    int kt, int tau_mode, int lpq, int m_pad, int splits, int k, int m, int n, const T *__restrict__ q,
    const T *__restrict__ r, const CandEntry *__restrict__ lists, const int *__restrict__ counts,
    const float *__restrict__ qnorm, DevScalars *__restrict__ scal, int64_t index_base,
    nns_key *__restrict__ keys, int *__restrict__ amb_list, int *__restrict__ multi_list, unsigned long long *__restrict__ diag)
{
    const int ush = lpq == 4 ? 4 : 5, qmask = (1 << ush) - 1;
    const int lane = threadIdx.x;
    const int unit = blockIdx.x;
    const int units = m_pad >> ush;
    const int i = (unit << ush) + (lane & qmask);
    const bool live = i < m;
    const unsigned long long d_r0 = __builtin_amdgcn_s_memrealtime();
    const unsigned long long d_t0 = k5_stamp();
    unsigned long long d_eval = 0;
    unsigned d_rounds = 0, d_active = 0;

    bool fallback = scal->q_maxabs_bits >= kHugeBits || refs_void(scal->r_maxabs_bits, tau_mode == TAU_F16);
    float a = __builtin_inff();
    int over = 0;
    if (!fallback && live) {
        for (int s = 0; s < splits; ++s) {
            const size_t lblk = (size_t)s * units + unit;
            const int cw = counts[lblk * 64 + lane];
            if (cw & kCandOverflow) over = 1;
            const int c = (cw & kCandCountMask) < kCandCap ? (cw & kCandCountMask) : kCandCap;
            const CandEntry *l = lists + lblk * (kCandCap * 64) + lane;
            for (int e = 0; e < c; ++e) a = fminf(a, l[e * 64].s);
        }
    }
    for (int off = 32; off >= (1 << ush); off >>= 1) {
        a = fminf(a, __shfl_xor(a, off, 64));
        over |= __shfl_xor(over, off, 64);
    }
    if (over || !(a < __builtin_inff())) fallback = true;
    const unsigned long long d_t1 = k5_stamp();

    nns_key best = NNS_KEY_NONE;
    int ncand = 0;
    {
        // (the walk runs to the wave's longest list, as a divergent loop does, so that the counters are the wave's)
        const bool walks = !fallback && live;
        float thr = 0.0f;
        if (walks) {
            const TauConsts tc = tau_consts(kt, qnorm[i], __uint_as_float(scal->ymax2_bits), tau_mode);
            thr = a + tau_of(tc, a);
        }
        const T *qi = q + (size_t)i * k;
        const bool vec = (k & 3) == 0 && (((uintptr_t)q | (uintptr_t)r) & (4 * sizeof(T) - 1)) == 0;
        for (int s = 0; s < splits; ++s) {
            const size_t lblk = (size_t)s * units + unit;
            int c = 0;
            if (walks) {
                const int cw = counts[lblk * 64 + lane] & kCandCountMask;
                c = cw < kCandCap ? cw : kCandCap;
            }
            const CandEntry *l = lists + lblk * (kCandCap * 64) + lane;
            int cmax = c;
            for (int off = 32; off > 0; off >>= 1) {
                const int o = __shfl_xor(cmax, off, 64);
                cmax = o > cmax ? o : cmax;
            }
            cmax = __builtin_amdgcn_readfirstlane(cmax);
            for (int e = 0; e < cmax; ++e) {
                CandEntry ce;
                ce.s = __builtin_inff();
                ce.j = n;
                if (e < c) ce = l[e * 64];
                const bool hit = e < c && ce.s <= thr && ce.j < n;
                const unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
                unsigned long long d_e0 = 0;
                if (mask) d_e0 = k5_stamp();
                if (hit) {
                    const float sum = v0_distance(qi, r + (size_t)ce.j * k, k, vec);
                    const nns_key key = make_key(sum, index_base + ce.j);
                    best = key < best ? key : best;
                    ++ncand;
                }
                if (mask) {
                    d_eval += k5_stamp() - d_e0;
                    ++d_rounds;
                    d_active += __builtin_popcountll(mask);
                }
            }
        }
    }
    const unsigned long long d_t2 = k5_stamp();
    for (int off = 32; off >= (1 << ush); off >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)best, off, 64);
        const unsigned hi = __shfl_xor((unsigned)(best >> 32), off, 64);
        const nns_key o = ((nns_key)hi << 32) | lo;
        best = o < best ? o : best;
        ncand += __shfl_xor(ncand, off, 64);
    }
    if (best == NNS_KEY_NONE) fallback = true;
    if (live && lane <= qmask) {
        keys[i] = fallback ? (nns_key)NNS_KEY_NONE : best;
        if (fallback) {
            const int pos = atomicAdd(&scal->amb_count, 1);
            amb_list[pos] = i;
        } else if (ncand > 1) {
            const int pos = atomicAdd(&scal->multi_count, 1);
            multi_list[pos] = i;
        }
    }
    if (diag) {
        // (the stamps are scalar: the wave's values, whichever lane stores them)
        if (lane == 0) {
            unsigned long long *o = diag + 8 * (size_t)unit;
            o[0] = d_t1 - d_t0;
            o[1] = d_t2 - d_t1;
            o[2] = d_eval;
            o[3] = d_rounds;
            o[4] = d_active;
            o[5] = __builtin_amdgcn_s_memrealtime() - d_r0;
        }
    }
}
#define K5_UNIT_KERNEL finalize_sparse_kernel
#define K5_UNIT_NAME "sparse"
#else
#define K5_UNIT_KERNEL finalize_kernel
#define K5_UNIT_NAME "compact"
#endif

// Same result, one WAVE per query: with many ref-range splits (few queries) a query owns
// 2 * splits candidate lists, and walking them from one thread serialises hundreds of
// dependent loads.  Lanes take lists l, l + 64, ...; the minimum score and the final key
// are reduced across the wave with packed-key / float shuffles.
//
// TILE RECORDS (FilterGeom.tile_rec, short ref streams): an entry is (minimum of the lane's scores of one ref tile,
// first ref of the lane's rows of that tile) — 16 rows j + 8 g + e (g, e < 4) of a 32 x 32 MFMA tile, 4 rows j + e of a
// 16 x 16 one.  The minimum over the entries is still the filter's minimum a of the query, and every ref with a score
// <= a + tau(a) sits in a tile whose minimum is <= a + tau(a): the members of C_i are among the rows of the entries
// within the threshold.  Each such entry is evaluated by 16 (4) lanes side by side, one row each, with V0's
// arithmetic; rows that are not in C_i take part in the exact minimum too, which cannot change V0's answer.
template <typename T>
__global__ __launch_bounds__(256) void finalize_wave_kernel(
    int kt, int tau_mode, int lpq, int tile_rec, int m_pad, int splits, int k, int m, int n, const T *__restrict__ q,
    const T *__restrict__ r, const CandEntry *__restrict__ lists, const int *__restrict__ counts,
    const float *__restrict__ qnorm, DevScalars *__restrict__ scal, int64_t index_base,
    nns_key *__restrict__ keys, int *__restrict__ amb_list, int *__restrict__ multi_list)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);   // wave-uniform query
    if (i >= m) return;
    const int nlists = lpq * splits;
    const int ush = lpq == 4 ? 4 : 5, qmask = (1 << ush) - 1, lsh = lpq == 4 ? 2 : 1;
    // (mode 4, fp16 points: a ref beyond kF16RefMax has no finite scaled operand — the host latch's twin)
    bool fallback = scal->q_maxabs_bits >= kHugeBits || refs_void(scal->r_maxabs_bits, tau_mode == TAU_F16);
    float a = __builtin_inff();
    int over = 0;
    for (int l = lane; l < nlists; l += 64) {
        const int s = l >> lsh, h = l & (lpq - 1);
        const size_t lblk = (size_t)s * (m_pad >> ush) + (i >> ush);
        const int ln = (h << ush) + (i & qmask);
        const int cw = counts[lblk * 64 + ln];
        if (cw & kCandOverflow) over = 1;
        const int c = (cw & kCandCountMask) < kCandCap ? (cw & kCandCountMask) : kCandCap;
        const CandEntry *lp = lists + lblk * (kCandCap * 64) + ln;
        for (int e = 0; e < c; ++e) a = fminf(a, lp[e * 64].s);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a = fminf(a, __shfl_xor(a, off, 64));
        over |= __shfl_xor(over, off, 64);
    }
    if (over || !(a < __builtin_inff())) fallback = true;

    nns_key best = NNS_KEY_NONE;
    int ncand = 0;
    if (!fallback) {
        const TauConsts tc = tau_consts(kt, qnorm[i], __uint_as_float(scal->ymax2_bits), tau_mode);
        const float thr = a + tau_of(tc, a);
        const T *qi = q + (size_t)i * k;
        const bool vec = (k & 3) == 0 && (((uintptr_t)q | (uintptr_t)r) & (4 * sizeof(T) - 1)) == 0;
        int over3 = 0;
        if (tile_rec) {
            // the lanes walk their lists in lockstep; an entry within the threshold is broadcast and its rows are
            // evaluated side by side, one lane per row (a V0 chain is sequential in t: the parallelism is over rows)
            const int nr = lpq == 4 ? 4 : 16;
            const int joff = lpq == 4 ? lane : (lane & 3) + 8 * (lane >> 2);
            for (int l0 = 0; l0 < nlists; l0 += 64) {
                const int l = l0 + lane;
                int c = 0;
                const CandEntry *lp = lists;
                if (l < nlists) {
                    const int s = l >> lsh, h = l & (lpq - 1);
                    const size_t lblk = (size_t)s * (m_pad >> ush) + (i >> ush);
                    const int ln = (h << ush) + (i & qmask);
                    const int cw = counts[lblk * 64 + ln] & kCandCountMask;
                    c = cw < kCandCap ? cw : kCandCap;
                    lp = lists + lblk * (kCandCap * 64) + ln;
                }
                int cmax = c;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    const int o = __shfl_xor(cmax, off, 64);
                    cmax = o > cmax ? o : cmax;
                }
                for (int e = 0; e < cmax; ++e) {
                    CandEntry ce;
                    ce.s = __builtin_inff();
                    ce.j = 0;
                    if (e < c) ce = lp[e * 64];
                    bool hit = e < c && ce.s <= thr;
                    // record form 2: entry 2 is the lane's THIRD-best tile minimum, with no tile attached — inside
                    // the threshold means more than two tiles of this lane's stream may hold V0's answer: exact scan
                    if (tile_rec == 2 && e == 2) {
                        if (hit) over3 = 1;
                        hit = false;
                    }
                    if (hit) ++ncand;   // (entries, i.e. tiles, within the threshold)
                    unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
                    while (mask) {      // (wave-uniform)
                        const int src = __builtin_ctzll(mask);
                        mask &= mask - 1;
                        const int j = __shfl(ce.j, src, 64) + joff;
                        if (lane < nr && j < n) {
                            const float sum = v0_distance(qi, r + (size_t)j * k, k, vec);
                            const nns_key key = make_key(sum, index_base + j);
                            best = key < best ? key : best;
                        }
                    }
                }
            }
        } else
        for (int l = lane; l < nlists; l += 64) {
            const int s = l >> lsh, h = l & (lpq - 1);
            const size_t lblk = (size_t)s * (m_pad >> ush) + (i >> ush);
            const int ln = (h << ush) + (i & qmask);
            const int cw = counts[lblk * 64 + ln] & kCandCountMask;
            const int c = cw < kCandCap ? cw : kCandCap;
            const CandEntry *lp = lists + lblk * (kCandCap * 64) + ln;
            for (int e = 0; e < c; ++e) {
                const CandEntry ce = lp[e * 64];
                if (ce.s <= thr && ce.j < n) {
                    const float sum = v0_distance(qi, r + (size_t)ce.j * k, k, vec);
                    const nns_key key = make_key(sum, index_base + ce.j);
                    best = key < best ? key : best;
                    ++ncand;
                }
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned lo = __shfl_xor((unsigned)best, off, 64);
            const unsigned hi = __shfl_xor((unsigned)(best >> 32), off, 64);
            const nns_key o = ((nns_key)hi << 32) | lo;
            best = o < best ? o : best;
            ncand += __shfl_xor(ncand, off, 64);
            over3 |= __shfl_xor(over3, off, 64);
        }
        if (best == NNS_KEY_NONE || over3) fallback = true;
    }
    if (lane == 0) {
        keys[i] = fallback ? (nns_key)NNS_KEY_NONE : best;
        if (fallback) {
            const int pos = atomicAdd(&scal->amb_count, 1);
            amb_list[pos] = i;
        } else if (ncand > 1) {
            const int pos = atomicAdd(&scal->multi_count, 1);
            multi_list[pos] = i;
        }
    }
}

// f(PointTag<T>{}) for the element type of the q / r that geometry g was planned for (the uint8 points' lists are the
// int8 image's, the re-rank reads the uint8 values; binary points have no filter: no K5 is built for them)
template <class F>
static int with_geom_type(const FilterGeom &g, F &&f)
{
    return with_point_type(g.dtype, [&](auto tag) {
        if constexpr (std::is_same_v<typename decltype(tag)::type, b1_t>) return (int)NNS_ERR_INVALID;
        else return f(tag);
    });
}

int launch_finalize(const FilterGeom &g, int k, int m, int n, const void *q, const void *r,
                    const CandEntry *lists, const int *counts, const float *qnorm, DevScalars *scal,
                    int64_t index_base, nns_key *keys, int *amb_list, int *multi_list, hipStream_t st)
{
    // (int8 and uint8 points: TAU_BF16 — exact scores, exact V0 distances, so its margin is a valid one)
    const int tau_mode = filter_tau_mode(g);
    if (g.splits >= 4) {   // few queries, many lists per query: one wave per query
        NNS_TRY(with_geom_type(g, [&](auto tag) {
            using T = typename decltype(tag)::type;
            hipLaunchKernelGGL(finalize_wave_kernel<T>, dim3(divup(m, 4)), dim3(256), 0, st, g.kt, tau_mode, g.lpq,
                               g.tile_rec, g.m_pad, g.splits, k, m, n, (const T *)q, (const T *)r, lists, counts, qnorm,
                               scal, index_base, keys, amb_list, multi_list);
            return (int)NNS_OK;
        }));
        NNS_HIP(hipGetLastError());
        return NNS_OK;
    }
    if (g.tile_rec) {   // (filter_plan couples tile records to splits >= 4)
        set_error("internal: tile records need the one-wave-per-query finalize");
        return NNS_ERR_INVALID;
    }
    const int units = g.m_pad / (64 / g.lpq);   // one 64-lane workgroup per list unit
#ifdef NNS_DIAG
    // NNS_K5_STAMPS=1: per-wave stamps of this launch, summed and printed as one JSON line on stderr (synchronous)
    unsigned long long *diag = nullptr;
    const char *want = getenv("NNS_K5_STAMPS");
    if (want && atoi(want)) {
        NNS_HIP(hipMalloc(&diag, (size_t)units * 8 * sizeof(unsigned long long)));
        NNS_HIP(hipMemsetAsync(diag, 0, (size_t)units * 8 * sizeof(unsigned long long), st));
    }
#endif
    NNS_TRY(with_geom_type(g, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(K5_UNIT_KERNEL<T>, dim3(units), dim3(64), 0, st, g.kt, tau_mode, g.lpq, g.m_pad, g.splits, k,
                           m, n, (const T *)q, (const T *)r, lists, counts, qnorm, scal, index_base, keys, amb_list,
                           multi_list K5_DIAG_ARG);
        return (int)NNS_OK;
    }));
#ifdef NNS_DIAG
    if (diag) {
        std::vector<unsigned long long> h((size_t)units * 8);
        NNS_HIP(hipGetLastError());
        NNS_HIP(hipStreamSynchronize(st));
        NNS_HIP(hipMemcpy(h.data(), diag, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        unsigned long long sum[6] = {0, 0, 0, 0, 0, 0};
        for (int u = 0; u < units; ++u)
            for (int f = 0; f < 6; ++f) sum[f] += h[(size_t)u * 8 + f];
        fprintf(stderr, "{\"k5_stamps\": \"%s\", \"units\": %d, \"splits\": %d, \"lpq\": %d, \"pass1_ticks\": %llu, "
                        "\"pass2_ticks\": %llu, \"eval_ticks\": %llu, \"eval_rounds\": %llu, \"eval_active_lanes\": %llu, "
                        "\"wave_realtime_ticks_100mhz\": %llu}\n",
                K5_UNIT_NAME, units, g.splits, g.lpq, sum[0], sum[1], sum[2], sum[3], sum[4], sum[5]);
        (void)hipFree(diag);
    }
#endif
    NNS_HIP(hipGetLastError());
    return NNS_OK;
}

}  // namespace nns
