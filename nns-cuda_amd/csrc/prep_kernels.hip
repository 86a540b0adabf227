// prep_kernels.hip — K2: the layout pre-pass in front of the MFMA filter.
//
// Role of the reference's mat_inv_kernel (core.cu:293-306 and its copies in
// v6..v9: AoS [n][k] -> SoA [k][n] so the fused kernel's loads coalesce) —
// re-designed for the MFMA operand feed of gfx950 instead of translated:
//
//   1. per-dimension mean c[t] of the reference shard (deterministic two-stage
//      reduction in fp64) — the clouds are centred before the -2*Q*R^T GEMM so
//      that |r'|^2 - 2 q'.r' loses as few bits as possible to cancellation
//      (SURVEY 7.3-1); correctness never depends on c, only the filter's
//      ambiguity margin tau does;
//   2. "tile image" of the centred (and, for refs, -2-scaled) points: per block of
//      32 points img[b][h][i][e] = v(point i, dim 8b+4h+e), the exact order in
//      which the 64 lanes of a wave consume float4 #b as operands of
//      v_mfma_f32_32x32x2_f32 k-steps 4b..4b+3.  One image block is 32*KT*4
//      contiguous bytes, so the filter's global->LDS DMA is a pure linear copy
//      and every ds_read_b128 of it is lane-linear (conflict-free);
//   3. squared norms of the centred points (fp64 accumulate, one fp32 rounding):
//      refs' norms seed the MFMA accumulators, queries' norms only enter tau;
//   4. max |value| and max norm (uint-ordered atomicMax on the fp32 bits), used to
//      bound the filter error and to detect NaN/INF/huge inputs, which are routed
//      to the exact kernels instead.
#include "nns_internal.h"

namespace nns {

constexpr int PREP_MEAN_BLOCKS = 1024;

// max-reduction into one device word: a plain read first (the word only grows), so that
// after the first few workgroups almost no atomic is issued — tens of thousands of
// workgroups hammering one address otherwise serialise the whole pre-pass
__device__ __forceinline__ void max_word(unsigned *word, unsigned v)
{
    if (v > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(word, v);
}

int prep_workspace_bytes(int kt, size_t *bytes)
{
    // (+ two floats per block and dimension: the minima and maxima the int8 pre-pass's scale comes from)
    *bytes = (size_t)PREP_MEAN_BLOCKS * kt * (sizeof(double) + 2 * sizeof(float));
    return NNS_OK;
}

// stage 1: per-block column sums.  Thread (rl, c4): c4 walks the dims four at a time (one
// 16-byte load per lane when k % 4 == 0), rl walks the rows, so a wave reads consecutive
// bytes.  Sums are fp64 in a fixed order -> the mean is deterministic.
// MM: also the block's per-dimension minimum and maximum -> minmax[blk][0 | 1][kt] (a dimension the block read nothing
// of: +INF, -INF)
template <int VEC, bool MM = false>
__global__ __launch_bounds__(256) void colsum_kernel(int k, int kt, int n, int rows_per_block,
                                                     const float *__restrict__ r,
                                                     double *__restrict__ partial,
                                                     unsigned *__restrict__ maxabs_bits,
                                                     float *__restrict__ minmax = nullptr)
{
    extern __shared__ double ssum[];   // [rl_count][kt] (MM: + [2][rl_count][kt] floats)
    const int cgroups = kt / VEC;                       // column groups per row
    const int cw = cgroups < 256 ? cgroups : 256;
    const int rl_count = 256 / cw;
    const int g0 = threadIdx.x % cw;
    const int rl = threadIdx.x / cw;
    const int row0 = blockIdx.x * rows_per_block;
    int row1 = row0 + rows_per_block;
    if (row1 > n) row1 = n;
    unsigned mx = 0;
    for (int g = g0; g < cgroups; g += cw) {
        double acc[VEC];
        float lo[VEC], hi[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            acc[e] = 0.0;
            lo[e] = INFINITY;
            hi[e] = -INFINITY;
        }
        const int c = g * VEC;
        if (c < k && rl < rl_count)
            for (int j = row0 + rl; j < row1; j += rl_count) {
                float v[VEC];
                if (VEC == 4) {
                    const float4 q = *reinterpret_cast<const float4 *>(r + (size_t)j * k + c);
                    v[0] = q.x;
                    v[VEC > 1 ? 1 : 0] = q.y;
                    v[VEC > 2 ? 2 : 0] = q.z;
                    v[VEC > 3 ? 3 : 0] = q.w;
                } else {
                    v[0] = r[(size_t)j * k + c];
                }
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    acc[e] += (double)v[e];
                    const unsigned b = __float_as_uint(v[e]) & 0x7FFFFFFFu;
                    mx = b > mx ? b : mx;
                    if constexpr (MM) {
                        lo[e] = fminf(lo[e], v[e]);
                        hi[e] = fmaxf(hi[e], v[e]);
                    }
                }
            }
        if (rl < rl_count)
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                ssum[rl * kt + c + e] = acc[e];
                if constexpr (MM) {
                    float *smm = reinterpret_cast<float *>(ssum + rl_count * kt);
                    smm[rl * kt + c + e] = lo[e];
                    smm[(rl_count + rl) * kt + c + e] = hi[e];
                }
            }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < kt; c += 256) {
        double acc = 0.0;
        for (int i = 0; i < rl_count; ++i) acc += ssum[i * kt + c];   // fixed order
        partial[(size_t)blockIdx.x * kt + c] = acc;
        if constexpr (MM) {
            const float *smm = reinterpret_cast<const float *>(ssum + rl_count * kt);
            float lo = INFINITY, hi = -INFINITY;
            for (int i = 0; i < rl_count; ++i) {
                lo = fminf(lo, smm[i * kt + c]);
                hi = fmaxf(hi, smm[(rl_count + i) * kt + c]);
            }
            minmax[((size_t)blockIdx.x * 2) * kt + c] = lo;
            minmax[((size_t)blockIdx.x * 2 + 1) * kt + c] = hi;
        }
    }
    // wave max then one atomic per wave
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        unsigned o = __shfl_xor(mx, off, 64);
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63) == 0) max_word(maxabs_bits, mx);
}

// stage 2: one workgroup per dimension, fixed-shape tree over the partials -> fp32 mean
// minmax / cmax_bits (the int8 pre-pass, both or neither): the dimension's extremes over the blocks, and the largest
// centred |coordinate| over the dimensions, max_t max(max_t - c_t, c_t - min_t) rounded up, as a uint-ordered max word
__global__ __launch_bounds__(256) void mean_kernel(int kt, int nblocks, int n, const double *__restrict__ partial,
                                                   float *__restrict__ mean, const float *__restrict__ minmax = nullptr,
                                                   unsigned *__restrict__ cmax_bits = nullptr)
{
    __shared__ double red[256];
    const int c = blockIdx.x;
    double acc = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256) acc += partial[(size_t)b * kt + c];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    const float mc = (float)(red[0] / (double)n);
    if (threadIdx.x == 0) mean[c] = mc;
    if (minmax) {
        __shared__ float rlo[256], rhi[256];
        float lo = INFINITY, hi = -INFINITY;
        for (int b = threadIdx.x; b < nblocks; b += 256) {
            lo = fminf(lo, minmax[((size_t)b * 2) * kt + c]);
            hi = fmaxf(hi, minmax[((size_t)b * 2 + 1) * kt + c]);
        }
        rlo[threadIdx.x] = lo;
        rhi[threadIdx.x] = hi;
        __syncthreads();
        for (int off = 128; off > 0; off >>= 1) {
            if (threadIdx.x < off) {
                rlo[threadIdx.x] = fminf(rlo[threadIdx.x], rlo[threadIdx.x + off]);
                rhi[threadIdx.x] = fmaxf(rhi[threadIdx.x], rhi[threadIdx.x + off]);
            }
            __syncthreads();
        }
        if (threadIdx.x == 0 && rlo[0] <= rhi[0]) {   // (a padding dimension has no values: centred 0)
            // the largest |y'| = |fl(y - c)| itself (the same subtraction), a few ulps up
            float d = fmaxf(__fsub_rn(rhi[0], mc), __fsub_rn(mc, rlo[0]));
            d = d * (1.0f + 0x1p-22f);
            if (!(d >= 0.0f)) d = INFINITY;   // (NaN coordinates: the scale is invalid)
            max_word(cmax_bits, __float_as_uint(d));
        }
    }
}

int launch_prep_mean(int k, int kt, int n, const float *r, double *partial_ws, float *mean,
                     unsigned *maxabs_bits, hipStream_t st, unsigned *cmax_bits)
{
    int nblocks = PREP_MEAN_BLOCKS;
    int rows = divup(n, nblocks);
    if (rows < 64) rows = 64;
    nblocks = divup(n, rows);
    const bool vec = (k % 4 == 0) && (((uintptr_t)r & 15) == 0);
    const int cgroups = vec ? kt / 4 : kt;
    const int cw = cgroups < 256 ? cgroups : 256;
    size_t lds = (size_t)(256 / cw) * kt * sizeof(double);
    float *minmax = reinterpret_cast<float *>(partial_ws + (size_t)PREP_MEAN_BLOCKS * kt);   // (behind the sums)
    if (cmax_bits) {
        lds += (size_t)(256 / cw) * kt * 2 * sizeof(float);
        if (vec)
            hipLaunchKernelGGL((colsum_kernel<4, true>), dim3(nblocks), dim3(256), lds, st, k, kt, n, rows, r, partial_ws,
                               maxabs_bits, minmax);
        else
            hipLaunchKernelGGL((colsum_kernel<1, true>), dim3(nblocks), dim3(256), lds, st, k, kt, n, rows, r, partial_ws,
                               maxabs_bits, minmax);
        NNS_HIP(hipGetLastError());
        hipLaunchKernelGGL(mean_kernel, dim3(kt), dim3(256), 0, st, kt, nblocks, n, partial_ws, mean, minmax, cmax_bits);
        NNS_HIP(hipGetLastError());
        return NNS_OK;
    }
    if (vec)
        hipLaunchKernelGGL(colsum_kernel<4>, dim3(nblocks), dim3(256), lds, st, k, kt, n, rows, r, partial_ws,
                           maxabs_bits, (float *)nullptr);
    else
        hipLaunchKernelGGL(colsum_kernel<1>, dim3(nblocks), dim3(256), lds, st, k, kt, n, rows, r, partial_ws,
                           maxabs_bits, (float *)nullptr);
    NNS_HIP(hipGetLastError());
    hipLaunchKernelGGL(mean_kernel, dim3(kt), dim3(256), 0, st, kt, nblocks, n, partial_ws, mean, (const float *)nullptr,
                       (unsigned *)nullptr);
    NNS_HIP(hipGetLastError());
    return NNS_OK;
}

// image kernel: one workgroup = one block of 32 points.
// BF = 1 (NNS_FILTER_BF16, fp32 points through the bf16 filter): the same centring and fp32 norms, but
// the image holds the centred, scaled values ROUNDED to bf16 (RNE) in the 16x16x32 operand order of
// image_bf16_kernel (order 1).  KT = 256 only.
// BF = 2 (split-bf16 operands, the filter's OpSplitT): the same centring and fp32 norms; every centred, scaled
// value v becomes h = rn_bf16(v) and l = rn_bf16(v - h) (v - h is exact in fp32), written as two 1 KiB
// fragments per 16-dim k-step in the v_mfma_f32_32x32x16_bf16 operand order (lane = 32 hl + i, dims
// 16 s + 8 hl .. + 7): fragment 2 s = hi, 2 s + 1 = lo.  The block keeps the fp32 image's bytes (KT / 8 fragments).
// I8 (the int8 pre-pass of a 128-deep lazy index, beside the BF = 3 / 2 image; I8PreArgs, nns_internal.h): the centred
// values once more as int8 under the shared scale s = cmax / 127 — v = y' / s, r8 = clamp(rint(v), +-127), e = v - r8 — in
// image_i8_kernel's lane map at depth 128 (fragment 2 t + ks: lane l holds dims 64 ks + 16 (l >> 4) .. + 15 of point
// 16 t + (l & 15)).  1 (refs): the image holds -r8, so that the filter's accumulator, seeded with N_j = floor(|y'_j|^2 /
// (2 s^2)), ends as N_j - q8.r8; max |r8|^2 and max |e_y|^2 go to their words.  2 (queries): q8 and the bound B8_i.
template <int KT, int BF, int I8>
__device__ __forceinline__ void image_body(int k, int npts, const float *__restrict__ pts,
                                           const float *__restrict__ mean, float scale,
                                           float pad_norm, float *__restrict__ img,
                                           float *__restrict__ norms,
                                           unsigned *__restrict__ max_norm_bits,
                                           unsigned *__restrict__ maxabs_bits, const I8PreArgs *x)
{
    constexpr int LD = KT + 4;                  // padded row (floats), keeps float4 alignment
    __shared__ __attribute__((aligned(16))) float tile[32 * LD];
    __shared__ double nrm[32][8];
    const int tid = threadIdx.x;
    const int blk = blockIdx.x;
    const int p0 = blk * 32;

    // load + centre: the 32 rows are one contiguous span of 32*k floats
    unsigned mx = 0;
    if ((k & 3) == 0 && k <= KT && p0 + 32 <= npts && (((uintptr_t)pts) & 15) == 0) {
        // full block of rows: 16-byte loads, consecutive lanes -> consecutive bytes (the 32 rows
        // are one contiguous span of 32 * k floats); dims k .. KT-1 are zero padding
        const int k4 = k >> 2;
        const float4 *src = reinterpret_cast<const float4 *>(pts + (size_t)p0 * k);
        const float4 *mean4 = reinterpret_cast<const float4 *>(mean);
        if (k < KT)
            for (int e = tid; e < 32 * (KT / 4); e += 256) {
                const int i = e / (KT / 4), t4 = e - i * (KT / 4);
                if (t4 >= k4) *reinterpret_cast<float4 *>(&tile[i * LD + 4 * t4]) = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        for (int e = tid; e < 32 * k4; e += 256) {
            const int i = e / k4, t4 = e - i * k4;
            const float4 v = src[e];
            const float4 mc = mean4[t4];
            const unsigned b0 = __float_as_uint(v.x) & 0x7FFFFFFFu, b1 = __float_as_uint(v.y) & 0x7FFFFFFFu;
            const unsigned b2 = __float_as_uint(v.z) & 0x7FFFFFFFu, b3 = __float_as_uint(v.w) & 0x7FFFFFFFu;
            const unsigned bm = max(max(b0, b1), max(b2, b3));
            mx = bm > mx ? bm : mx;
            float4 c;   // ONE rounding each: x' = fl(x - c)
            c.x = __fsub_rn(v.x, mc.x);
            c.y = __fsub_rn(v.y, mc.y);
            c.z = __fsub_rn(v.z, mc.z);
            c.w = __fsub_rn(v.w, mc.w);
            *reinterpret_cast<float4 *>(&tile[i * LD + 4 * t4]) = c;
        }
    } else {
        for (int e = tid; e < 32 * KT; e += 256) {
            const int i = e / KT, t = e - i * KT;
            float c = 0.0f;
            if (t < k && p0 + i < npts) {
                const float v = pts[(size_t)(p0 + i) * k + t];
                const unsigned b = __float_as_uint(v) & 0x7FFFFFFFu;
                mx = b > mx ? b : mx;
                c = __fsub_rn(v, mean[t]);   // ONE rounding: x' = fl(x - c)
            }
            tile[i * LD + t] = c;
        }
    }
    __syncthreads();

    // squared norm of the centred row: 8 threads per row, fp64, fixed order
    {
        const int i = tid >> 3, part = tid & 7;
        double acc = 0.0;
        for (int t = part; t < KT; t += 8) {
            const double v = (double)tile[i * LD + t];
            acc += v * v;
        }
        nrm[i][part] = acc;
    }
    __syncthreads();
    double nsq = 0.0;   // (I8: the row's squared norm once more, for the seed)
    if (tid < 32) {
        double acc = 0.0;
        for (int p = 0; p < 8; ++p) acc += nrm[tid][p];
        nsq = acc;
        float nv = (float)acc;
        unsigned nb = 0;
        if (p0 + tid >= npts) nv = pad_norm;           // padding never wins (refs: +INF)
        else nb = __float_as_uint(nv);
        norms[p0 + tid] = nv;
        if (max_norm_bits) {                           // block max (lanes 0..31), one update
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) {
                const unsigned o = __shfl_xor(nb, off, 64);
                nb = o > nb ? o : nb;
            }
            if (tid == 0) max_word(max_norm_bits, nb);
        }
    }

    if constexpr (BF == 2 || BF == 3) {
        // BF = 3, the lazy layout of the same values: fragment s of the block's hi parts at [blk][s], of its lo parts at
        // [gridDim.x + blk][s] (one launch covers the whole padded point set: gridDim.x blocks), KT / 16 fragments each
        uint4 *outb = reinterpret_cast<uint4 *>(img + (BF == 2 ? (size_t)blk * 32 * KT : 0));
        for (int f = tid; f < (KT / 8) * 64; f += 256) {
            const int s2 = f >> 6, lane = f & 63;
            const int i = lane & 31, d0 = 16 * (s2 >> 1) + 8 * (lane >> 5);
            const bool lo_part = (s2 & 1) != 0;
            unsigned w[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                unsigned short p[2];
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const float v = tile[i * LD + d0 + 2 * e + c] * scale;   // scale +1 / -2: exact
                    const __bf16 hv = (__bf16)v;                              // RNE; NaN stays NaN
                    p[c] = __builtin_bit_cast(unsigned short, lo_part ? (__bf16)__fsub_rn(v, (float)hv) : hv);
                }
                w[e] = (unsigned)p[0] | ((unsigned)p[1] << 16);
            }
            if constexpr (BF == 3)
                outb[(((lo_part ? (size_t)gridDim.x : 0) + blk) * (KT / 16) + (s2 >> 1)) * 64 + lane] = make_uint4(w[0], w[1], w[2], w[3]);
            else
                outb[f] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    } else if constexpr (BF != 0) {
        static_assert(BF == 1, "BF 2 / 3 are handled above");
        static_assert(BF == 0 || KT == 256 || KT == 128, "the bf16 operand image is 128 or 256 deep");
        // fragment f = NKS * tile + k-step; lane l: point 16 tile + (l & 15), dims 32 ks + 8 (l >> 4) .. + 7
        constexpr int NKS = KT / 32;
        uint4 *outb = reinterpret_cast<uint4 *>(reinterpret_cast<uint16_t *>(img) + (size_t)blk * 32 * KT);
        for (int f = tid; f < 2 * NKS * 64; f += 256) {
            const int s16 = f >> 6, lane = f & 63;
            const int i = 16 * (s16 / NKS) + (lane & 15), d0 = 32 * (s16 % NKS) + 8 * (lane >> 4);
            unsigned w[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                // scale (+1 / -2) is exact in fp32 and in bf16; ONE rounding to bf16, NaN stays NaN
                const __bf16 lo = (__bf16)(tile[i * LD + d0 + 2 * e] * scale);
                const __bf16 hi = (__bf16)(tile[i * LD + d0 + 2 * e + 1] * scale);
                w[e] = (unsigned)__builtin_bit_cast(unsigned short, lo) |
                       ((unsigned)__builtin_bit_cast(unsigned short, hi) << 16);
            }
            outb[f] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    } else {
    // write the image: float4 #f of the block = img[b][lane][0..3], lane = 32h + i
    float4 *out = reinterpret_cast<float4 *>(img + (size_t)blk * 32 * KT);
    for (int f = tid; f < (KT / 8) * 64; f += 256) {
        const int b = f >> 6, lane = f & 63;
        const int h = lane >> 5, i = lane & 31;
        const float4 v = *reinterpret_cast<const float4 *>(&tile[i * LD + 8 * b + 4 * h]);
        float4 o;
        o.x = v.x * scale;   // scale is +1 or -2: exact
        o.y = v.y * scale;
        o.z = v.z * scale;
        o.w = v.w * scale;
        out[f] = o;
    }
    }

#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        unsigned o = __shfl_xor(mx, off, 64);
        mx = o > mx ? o : mx;
    }
    if ((tid & 63) == 0 && maxabs_bits) max_word(maxabs_bits, mx);

    if constexpr (I8 != 0) {
        static_assert(KT == 128, "the int8 pre-pass is 128 deep: four fragments per block, one per wave");
        __shared__ float pe2[32][8];
        __shared__ int pr2[32][8];
        const float cmax = __uint_as_float(x->scal->i8_cmax_bits);
        const bool valid = i8pre_scale_valid(x->scal->i8_cmax_bits);   // (all refs equal, INF / NaN / huge: no scale)
        const float s = cmax / 127.0f;
        const float inv = valid ? 127.0f / cmax : 0.0f;
        const int frag = tid >> 6, lane = tid & 63;
        const int i = 16 * (frag >> 1) + (lane & 15), d0 = 64 * (frag & 1) + 16 * (lane >> 4);
        unsigned w[4];
        float e2 = 0.0f;
        int r2 = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            w[e] = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const float v = tile[i * LD + d0 + 4 * e + b] * inv;
                const float r = fminf(fmaxf(rintf(v), -127.0f), 127.0f);   // (NaN -> -127: such inputs never reach the filter's answer)
                const float d = v - r;
                e2 += d * d;
                const int ri = (int)r;
                r2 += ri * ri;
                w[e] |= (unsigned)(unsigned char)(int8_t)(I8 == 1 ? -ri : ri) << (8 * b);
            }
        }
        x->img8[(size_t)blk * 256 + tid] = make_uint4(w[0], w[1], w[2], w[3]);
        pe2[i][4 * (frag & 1) + (lane >> 4)] = e2;
        pr2[i][4 * (frag & 1) + (lane >> 4)] = r2;
        __syncthreads();
        if (tid < 32) {
            float es = 0.0f;
            int rs = 0;
            for (int p = 0; p < 8; ++p) {
                es += pe2[tid][p];
                rs += pr2[tid][p];
            }
            es *= 1.0f + 0x1p-20f;   // (the fp32 sum of 128 squares, rounded up)
            const bool live = p0 + tid < npts;
            if constexpr (I8 == 1) {
                int seed = kI8PrePadSeed;
                if (live && valid) {
                    const double q = nsq / (2.0 * (double)s * (double)s);
                    seed = q < (double)kI8PreThrMax ? (int)q : kI8PrePadSeed;   // (floor of a value >= 0)
                }
                x->seeds[p0 + tid] = seed;
                unsigned eb = live ? __float_as_uint(es) : 0u, rb = live ? __float_as_uint((float)rs) : 0u;
#pragma unroll
                for (int off = 16; off > 0; off >>= 1) {
                    const unsigned oe = __shfl_xor(eb, off, 64), orr = __shfl_xor(rb, off, 64);
                    eb = oe > eb ? oe : eb;
                    rb = orr > rb ? orr : rb;
                }
                if (tid == 0) {
                    max_word(&x->scal->i8_eymax2_bits, eb);
                    max_word(&x->scal->i8_r8max2_bits, rb);
                }
            } else {
                const float c0 = tau_consts(KT, (float)nsq, __uint_as_float(x->scal->ymax2_bits), 3).c0;
                const float b8 = valid ? i8pre_bound(s, es, (float)rs, __uint_as_float(x->scal->i8_r8max2_bits),
                                                     __uint_as_float(x->scal->i8_eymax2_bits), c0)
                                       : INFINITY;
                x->bound[p0 + tid] = b8;
                // the selection rule's count (an integer sum: the same whatever the order)
                const bool odd = live && !(b8 <= 1.5f * split_lazy_bound(KT, (float)nsq, __uint_as_float(x->scal->ymax2_bits)));
                const unsigned long long om = __builtin_amdgcn_ballot_w64(odd);
                if (tid == 0 && om != 0ull) atomicAdd(&x->scal->i8_odd_count, __builtin_popcountll(om));
            }
        }
    }
}

template <int KT, int BF = 0>
__global__ __launch_bounds__(256) void image_kernel(int k, int npts, const float *__restrict__ pts,
                                                    const float *__restrict__ mean, float scale,
                                                    float pad_norm, float *__restrict__ img,
                                                    float *__restrict__ norms,
                                                    unsigned *__restrict__ max_norm_bits,
                                                    unsigned *__restrict__ maxabs_bits)
{
    image_body<KT, BF, 0>(k, npts, pts, mean, scale, pad_norm, img, norms, max_norm_bits, maxabs_bits, nullptr);
}
// ... with the int8 pre-pass's operands (I8 = 1 refs beside the lazy image, 2 queries beside the split image)
template <int BF, int I8>
__global__ __launch_bounds__(256) void image_i8pre_kernel(int k, int npts, const float *__restrict__ pts,
                                                          const float *__restrict__ mean, float scale,
                                                          float pad_norm, float *__restrict__ img,
                                                          float *__restrict__ norms,
                                                          unsigned *__restrict__ max_norm_bits,
                                                          unsigned *__restrict__ maxabs_bits, const I8PreArgs x)
{
    image_body<128, BF, I8>(k, npts, pts, mean, scale, pad_norm, img, norms, max_norm_bits, maxabs_bits, &x);
}

// NNS_FILTER_BF16 at KT = 512 (fp32 points, 256 < k <= 512; operands in the 32x32x16 order 0 of
// image_bf16_kernel): the fp32 tile of image_kernel would not fit the 64 KiB of static LDS, so
// each thread centres, squares (fp64) and rounds a 64-dim run of one point on the fly and only
// the bf16 values are staged.  Same values as image_kernel<KT, 1> would produce.
__global__ __launch_bounds__(256) void image_mixed512_kernel(int order, int k, int npts, const float *__restrict__ pts,
                                                             const float *__restrict__ mean, float scale,
                                                             float pad_norm, uint16_t *__restrict__ img,
                                                             float *__restrict__ norms,
                                                             unsigned *__restrict__ max_norm_bits,
                                                             unsigned *__restrict__ maxabs_bits)
{
    constexpr int KT = 512, LD = KT + 8;
    __shared__ __attribute__((aligned(16))) uint16_t tile[32 * LD];
    __shared__ double nrm[32][8];
    const int tid = threadIdx.x;
    const int blk = blockIdx.x;
    const int p0 = blk * 32;
    const int i = tid >> 3, part = tid & 7;   // 8 threads per point, 64 consecutive dims each
    const bool live = p0 + i < npts;
    const float *row = pts + (size_t)(p0 + i) * k;
    unsigned mx = 0;
    double acc = 0.0;
    for (int t = part * 64; t < part * 64 + 64; ++t) {
        float c = 0.0f;
        if (live && t < k) {
            const float v = row[t];
            const unsigned b = __float_as_uint(v) & 0x7FFFFFFFu;
            mx = b > mx ? b : mx;
            c = __fsub_rn(v, mean[t]);   // ONE rounding: x' = fl(x - c)
        }
        acc += (double)c * (double)c;
        // scale (+1 / -2) is exact; ONE rounding to bf16 (RNE), NaN stays NaN
        tile[i * LD + t] = __builtin_bit_cast(unsigned short, (__bf16)(c * scale));
    }
    nrm[i][part] = acc;
    __syncthreads();
    if (tid < 32) {
        double a2 = 0.0;
        for (int p = 0; p < 8; ++p) a2 += nrm[tid][p];   // fixed order
        float nv = (float)a2;
        unsigned nb = 0;
        if (p0 + tid >= npts) nv = pad_norm;             // padding never wins (refs: +INF)
        else nb = __float_as_uint(nv);
        norms[p0 + tid] = nv;
        if (max_norm_bits) {
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) {
                const unsigned o = __shfl_xor(nb, off, 64);
                nb = o > nb ? o : nb;
            }
            if (tid == 0) max_word(max_norm_bits, nb);
        }
    }
    // 16-byte fragments: f = s * 64 + lane.  order 0 (32x32x16 operands): lane = 32 h + i, dims 16 s + 8 h ..;
    // order 1 (16x16x32 operands): fragment (KT / 32) t + ks, lane: point 16 t + (l & 15), dims 32 ks + 8 (l >> 4) ..
    uint4 *out = reinterpret_cast<uint4 *>(img + (size_t)blk * 32 * KT);
    for (int f = tid; f < (KT / 16) * 64; f += 256) {
        const int s16 = f >> 6, lane = f & 63;
        int i, d0;
        if (order == 0) {
            i = lane & 31;
            d0 = 16 * s16 + 8 * (lane >> 5);
        } else {
            constexpr int NKS = KT / 32;
            i = 16 * (s16 / NKS) + (lane & 15);
            d0 = 32 * (s16 % NKS) + 8 * (lane >> 4);
        }
        out[f] = *reinterpret_cast<const uint4 *>(&tile[i * LD + d0]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        unsigned o = __shfl_xor(mx, off, 64);
        mx = o > mx ? o : mx;
    }
    if ((tid & 63) == 0 && maxabs_bits) max_word(maxabs_bits, mx);
}

// KT = 1024 (512 < k <= 1024), operands of v_mfma_f32_32x32x16_bf16 (order 0), for BOTH point types: a
// 32-point block is 64 KiB of bf16 — more than one staging tile — so the block is produced in two halves of
// 512 dims through the same LDS tile; the squared norm accumulates in a register across the halves (fp64,
// fixed order).  T = float: centred by the mean, ONE rounding to bf16 (NNS_FILTER_BF16 / AUTO for fp32 points
// beyond the fp32 tiles); T = uint16_t: bf16 bit patterns, no centring (a centred bf16 value would need a
// second rounding).  Same values as image_mixed512_kernel / image_bf16_kernel would produce at their depths.
// (KT = 768: three parts of 256 dims; KT = 640 / 384: five / three parts of 128.)
template <int KT, typename T, int HD = 512>
__global__ __launch_bounds__(256) void image_deep_kernel(int k, int npts, const T *__restrict__ pts,
                                                         const float *__restrict__ mean, float scale, float pad_norm,
                                                         uint16_t *__restrict__ img, float *__restrict__ norms,
                                                         unsigned *__restrict__ max_norm_bits,
                                                         unsigned *__restrict__ maxabs_bits)
{
    static_assert(KT % HD == 0 && HD % 64 == 0, "parts of HD dims, 8 threads per point");
    constexpr int LD = HD + 8, TPD = HD / 8;   // dims per thread and part
    __shared__ __attribute__((aligned(16))) uint16_t tile[32 * LD];
    __shared__ double nrm[32][8];
    const int tid = threadIdx.x;
    const int blk = blockIdx.x;
    const int p0 = blk * 32;
    const int i = tid >> 3, part = tid & 7;   // 8 threads per point, 64 consecutive dims each per half
    const bool live = p0 + i < npts;
    const T *row = pts + (size_t)(p0 + i) * k;
    unsigned mx = 0;
    double acc = 0.0;
    uint4 *out = reinterpret_cast<uint4 *>(img + (size_t)blk * 32 * KT);
    for (int half = 0; half < KT / HD; ++half) {
        for (int tt = part * TPD; tt < part * TPD + TPD; ++tt) {
            const int t = half * HD + tt;
            float c = 0.0f;
            if (live && t < k) {
                float v;
                if constexpr (sizeof(T) == 4) v = (float)row[t];
                else v = __uint_as_float((unsigned)row[t] << 16);
                const unsigned b = __float_as_uint(v) & 0x7FFFFFFFu;
                mx = b > mx ? b : mx;
                if constexpr (sizeof(T) == 4) c = __fsub_rn(v, mean[t]);   // ONE rounding: x' = fl(x - c)
                else c = v;
            }
            acc += (double)c * (double)c;
            // scale (+1 / -2) is exact; fp32 points: ONE rounding to bf16 (RNE), NaN stays NaN; bf16 points: exact
            tile[i * LD + tt] = __builtin_bit_cast(unsigned short, (__bf16)(c * scale));
        }
        __syncthreads();
        // 16-byte fragments of the 32x32x16 operand order: fragment s (16 dims), lane = 32 h + i
        for (int f = tid; f < (HD / 16) * 64; f += 256) {
            const int s16 = f >> 6, lane = f & 63;
            out[(half * (HD / 16) + s16) * 64 + lane] =
                *reinterpret_cast<const uint4 *>(&tile[(lane & 31) * LD + 16 * s16 + 8 * (lane >> 5)]);
        }
        __syncthreads();
    }
    nrm[i][part] = acc;
    __syncthreads();
    if (tid < 32) {
        double a2 = 0.0;
        for (int p = 0; p < 8; ++p) a2 += nrm[tid][p];   // fixed order
        float nv = (float)a2;
        unsigned nb = 0;
        if (p0 + tid >= npts) nv = pad_norm;             // padding never wins (refs: +INF)
        else nb = __float_as_uint(nv);
        norms[p0 + tid] = nv;
        if (max_norm_bits) {
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) {
                const unsigned o = __shfl_xor(nb, off, 64);
                nb = o > nb ? o : nb;
            }
            if (tid == 0) max_word(max_norm_bits, nb);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        unsigned o = __shfl_xor(mx, off, 64);
        mx = o > mx ? o : mx;
    }
    if ((tid & 63) == 0 && maxabs_bits) max_word(maxabs_bits, mx);
}

// form: 0 fp32 image, 1 bf16-rounded operands, 2 split-bf16 operands (hi, lo fragment per k-step), 3 the same values in
// the lazy layout: the hi fragments of all blocks ([npts_pad / 32][kt / 16] KiB), then the lo fragments likewise
static int launch_prep_image(int k, int kt, int npts, int npts_pad, const float *pts, const float *mean,
                             float scale, float pad_norm, float *img, float *norms,
                             unsigned *max_norm_bits, unsigned *maxabs_bits, hipStream_t st, int form, const I8PreArgs *i8)
{
    const int blocks = npts_pad / 32;
    if (i8) {   // refs (form 3) or queries (form 2) of a 128-deep lazy index, with the int8 pre-pass's operands
        if (kt != 128 || (form != 3 && form != 2)) {
            set_error("prep: the int8 pre-pass goes with the split image at tile K 128 (kt = %d, form %d)", kt, form);
            return NNS_ERR_UNSUPPORTED;
        }
        if (form == 3)
            hipLaunchKernelGGL((image_i8pre_kernel<3, 1>), dim3(blocks), dim3(256), 0, st, k, npts, pts, mean, scale, pad_norm,
                               img, norms, max_norm_bits, maxabs_bits, *i8);
        else
            hipLaunchKernelGGL((image_i8pre_kernel<2, 2>), dim3(blocks), dim3(256), 0, st, k, npts, pts, mean, scale, pad_norm,
                               img, norms, max_norm_bits, maxabs_bits, *i8);
        NNS_HIP(hipGetLastError());
        return NNS_OK;
    }
    if (form == 3) {   // split-bf16 operands in the lazy layout (the depths of the lazy kernel)
        if (kt != 128) {
            set_error("prep: the lazy split layout is built at tile K 128 only (kt = %d)", kt);
            return NNS_ERR_UNSUPPORTED;
        }
        hipLaunchKernelGGL((image_kernel<128, 3>), dim3(blocks), dim3(256), 0, st, k, npts, pts, mean, scale, pad_norm, img,
                           norms, max_norm_bits, maxabs_bits);
        NNS_HIP(hipGetLastError());
        return NNS_OK;
    }
    if (form == 2) {   // split-bf16 operands at the fp32 depths
        switch (kt) {
        case 16:
            hipLaunchKernelGGL((image_kernel<16, 2>), dim3(blocks), dim3(256), 0, st, k, npts, pts, mean, scale, pad_norm, img,
                               norms, max_norm_bits, maxabs_bits);
            break;
        case 32:
            hipLaunchKernelGGL((image_kernel<32, 2>), dim3(blocks), dim3(256), 0, st, k, npts, pts, mean, scale, pad_norm, img,
                               norms, max_norm_bits, maxabs_bits);
            break;
        case 64:
            hipLaunchKernelGGL((image_kernel<64, 2>), dim3(blocks), dim3(256), 0, st, k, npts, pts, mean, scale, pad_norm, img,
                               norms, max_norm_bits, maxabs_bits);
            break;
        case 128:
            hipLaunchKernelGGL((image_kernel<128, 2>), dim3(blocks), dim3(256), 0, st, k, npts, pts, mean, scale, pad_norm, img,
                               norms, max_norm_bits, maxabs_bits);
            break;
        case 256:
            hipLaunchKernelGGL((image_kernel<256, 2>), dim3(blocks), dim3(256), 0, st, k, npts, pts, mean, scale, pad_norm, img,
                               norms, max_norm_bits, maxabs_bits);
            break;
        default:
            set_error("prep: unsupported split-operand tile K %d", kt);
            return NNS_ERR_UNSUPPORTED;
        }
        NNS_HIP(hipGetLastError());
        return NNS_OK;
    }
    if (form == 1) {
        if (kt != 1024 && kt != 768 && kt != 640 && kt != 512 && kt != 384 && kt != 256 && kt != 128) {
            set_error("prep: the bf16 operand image is 128, 256, 384, 512, 640, 768 or 1024 deep (kt = %d)", kt);
            return NNS_ERR_UNSUPPORTED;
        }
        if (kt == 384)
            hipLaunchKernelGGL((image_deep_kernel<384, float, 128>), dim3(blocks), dim3(256), 0, st, k, npts, pts, mean, scale,
                               pad_norm, (uint16_t *)img, norms, max_norm_bits, maxabs_bits);
        else if (kt == 640)
            hipLaunchKernelGGL((image_deep_kernel<640, float, 128>), dim3(blocks), dim3(256), 0, st, k, npts, pts, mean, scale,
                               pad_norm, (uint16_t *)img, norms, max_norm_bits, maxabs_bits);
        else if (kt == 768)
            hipLaunchKernelGGL((image_deep_kernel<768, float, 256>), dim3(blocks), dim3(256), 0, st, k, npts, pts, mean, scale,
                               pad_norm, (uint16_t *)img, norms, max_norm_bits, maxabs_bits);
        else if (kt == 1024)
            hipLaunchKernelGGL((image_deep_kernel<1024, float>), dim3(blocks), dim3(256), 0, st, k, npts, pts, mean, scale,
                               pad_norm, (uint16_t *)img, norms, max_norm_bits, maxabs_bits);
        else if (kt == 512)
            hipLaunchKernelGGL(image_mixed512_kernel, dim3(blocks), dim3(256), 0, st, kBf16ImageOrder, k, npts, pts, mean,
                               scale, pad_norm, (uint16_t *)img, norms, max_norm_bits, maxabs_bits);
        else if (kt == 256)
            hipLaunchKernelGGL((image_kernel<256, 1>), dim3(blocks), dim3(256), 0, st, k, npts, pts, mean, scale,
                               pad_norm, img, norms, max_norm_bits, maxabs_bits);
        else
            hipLaunchKernelGGL((image_kernel<128, 1>), dim3(blocks), dim3(256), 0, st, k, npts, pts, mean, scale,
                               pad_norm, img, norms, max_norm_bits, maxabs_bits);
        NNS_HIP(hipGetLastError());
        return NNS_OK;
    }
    switch (kt) {
    case 16:
        hipLaunchKernelGGL(image_kernel<16>, dim3(blocks), dim3(256), 0, st, k, npts, pts, mean,
                           scale, pad_norm, img, norms, max_norm_bits, maxabs_bits);
        break;
    case 32:
        hipLaunchKernelGGL(image_kernel<32>, dim3(blocks), dim3(256), 0, st, k, npts, pts, mean,
                           scale, pad_norm, img, norms, max_norm_bits, maxabs_bits);
        break;
    case 64:
        hipLaunchKernelGGL(image_kernel<64>, dim3(blocks), dim3(256), 0, st, k, npts, pts, mean,
                           scale, pad_norm, img, norms, max_norm_bits, maxabs_bits);
        break;
    case 128:
        hipLaunchKernelGGL(image_kernel<128>, dim3(blocks), dim3(256), 0, st, k, npts, pts, mean,
                           scale, pad_norm, img, norms, max_norm_bits, maxabs_bits);
        break;
    case 256:
        hipLaunchKernelGGL(image_kernel<256>, dim3(blocks), dim3(256), 0, st, k, npts, pts, mean,
                           scale, pad_norm, img, norms, max_norm_bits, maxabs_bits);
        break;
    default:
        set_error("prep: unsupported tile K %d", kt);
        return NNS_ERR_UNSUPPORTED;
    }
    NNS_HIP(hipGetLastError());
    return NNS_OK;
}

// ---- bf16 image (K4's operands) --------------------------------------------------------
// One workgroup = one block of 32 points, KT = 256.  The image is [16 steps][64 lanes][8 bf16]:
// lane (i = lane & 31, h = lane >> 5) of step s holds dims 16s + 8h .. 16s + 8h + 7 of point
// i — one v_mfma_f32_32x32x16_bf16 operand per ds_read_b128.  No centring (a centred bf16
// value would need a second rounding); the scale (-2 for refs) is exact in bf16.
//
// order 1 (v_mfma_f32_16x16x32_bf16 operands, the product): a fragment is one 16-point tile t x
// one k-step ks of 32 dims; lane l holds dims 32 ks + 8 (l >> 4) .. + 7 of point 16 t + (l & 15);
// the block stores fragment (KT / 32) t + ks (the filter walks a ref tile's k-steps in a row; a wave
// keeps all k-steps of its four query tiles in registers).  order 0: the 32x32x16 layout above.
//
// F16 (fp16 points, order 1, KT = 128 / 256: v_mfma_f32_16x16x32_f16 operands): the same permutation of 16-bit words.
// Values are widened with v_cvt_f32_f16 for the fp64 norms and for the max-|v| word (kept as fp32 bits, so the host's and
// K5's comparisons read it like the other types'), and the scaled value is narrowed with a real conversion: -2 v is
// exact in binary16 for |v| <= 32752 (subnormals included: doubling is exact); beyond, the image holds INF and the
// max-|v| word voids the filter (kF16RefMax, nns_internal.h).
template <int KT, bool F16 = false>
__global__ __launch_bounds__(256) void image_bf16_kernel(int order, int k, int npts, const uint16_t *__restrict__ pts,
                                                         float scale, float pad_norm,
                                                         uint16_t *__restrict__ img, float *__restrict__ norms,
                                                         unsigned *__restrict__ max_norm_bits,
                                                         unsigned *__restrict__ maxabs_bits)
{
    constexpr int LD = KT + 8, NKS = KT / 32;
    __shared__ __attribute__((aligned(16))) uint16_t tile[32 * LD];
    __shared__ double nrm[32][8];
    const int tid = threadIdx.x;
    const int blk = blockIdx.x;
    const int p0 = blk * 32;
    unsigned mx = 0;
    if (k == KT && p0 + 32 <= npts && (((uintptr_t)pts) & 15) == 0) {
        const uint4 *src = reinterpret_cast<const uint4 *>(pts + (size_t)p0 * KT);   // 8 bf16 per load
        for (int e = tid; e < 32 * (KT / 8); e += 256) {
            const int i = e / (KT / 8), t8 = e - i * (KT / 8);
            const uint4 v = src[e];
            const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                unsigned lo, hi;
                if constexpr (F16) {
                    lo = __float_as_uint(f16_widen_lo(w[u] & 0x7FFF7FFFu));
                    hi = __float_as_uint(f16_widen_hi(w[u] & 0x7FFF7FFFu));
                } else {
                    lo = (w[u] << 16) & 0x7FFFFFFFu;
                    hi = w[u] & 0x7FFF0000u;
                }
                mx = max(mx, max(lo, hi));
            }
            *reinterpret_cast<uint4 *>(&tile[i * LD + 8 * t8]) = v;
        }
    } else {
        for (int e = tid; e < 32 * KT; e += 256) {
            const int i = e / KT, t = e - i * KT;
            uint16_t v = 0;
            if (t < k && p0 + i < npts) {
                v = pts[(size_t)(p0 + i) * k + t];
                const unsigned b = F16 ? __float_as_uint(f16_widen(v & 0x7FFFu)) : ((unsigned)v << 16) & 0x7FFFFFFFu;
                mx = b > mx ? b : mx;
            }
            tile[i * LD + t] = v;
        }
    }
    __syncthreads();
    {
        const int i = tid >> 3, part = tid & 7;
        double acc = 0.0;
        for (int t = part; t < KT; t += 8) {
            const double v = (double)(F16 ? f16_widen(tile[i * LD + t]) : __uint_as_float((unsigned)tile[i * LD + t] << 16));
            acc += v * v;
        }
        nrm[i][part] = acc;
    }
    __syncthreads();
    if (tid < 32) {
        double acc = 0.0;
        for (int p = 0; p < 8; ++p) acc += nrm[tid][p];
        float nv = (float)acc;
        unsigned nb = 0;
        if (p0 + tid >= npts) nv = pad_norm;
        else nb = __float_as_uint(nv);
        norms[p0 + tid] = nv;
        if (max_norm_bits) {
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) {
                const unsigned o = __shfl_xor(nb, off, 64);
                nb = o > nb ? o : nb;
            }
            if (tid == 0) max_word(max_norm_bits, nb);
        }
    }
    // 16-byte fragments: f = s * 64 + lane
    uint4 *out = reinterpret_cast<uint4 *>(img + (size_t)blk * 32 * KT);
    for (int f = tid; f < (KT / 16) * 64; f += 256) {
        const int s = f >> 6, lane = f & 63;
        int i, d0;   // point of the block and first dim of this lane's 8
        if (order == 0) {
            i = lane & 31;
            d0 = 16 * s + 8 * (lane >> 5);
        } else {
            const int t = s / NKS, ks = s % NKS;
            i = 16 * t + (lane & 15);
            d0 = 32 * ks + 8 * (lane >> 4);
        }
        const uint4 sv = *reinterpret_cast<const uint4 *>(&tile[i * LD + d0]);
        const unsigned in[4] = {sv.x, sv.y, sv.z, sv.w};
        unsigned w[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if constexpr (F16) {
                // scale in fp32, ONE conversion back to binary16: exact for scale in {1, -2} while |v| <= 32752
                w[e] = f16_narrow(f16_widen_lo(in[e]) * scale) | (f16_narrow(f16_widen_hi(in[e]) * scale) << 16);
                continue;
            }
            // scale in fp32 and narrow back: exact for scale in {1, -2} (no overflow below 1e17)
            const float lo = __uint_as_float(in[e] << 16) * scale;
            const float hi = __uint_as_float(in[e] & 0xFFFF0000u) * scale;
            w[e] = (__float_as_uint(lo) >> 16) | (__float_as_uint(hi) & 0xFFFF0000u);
        }
        out[f] = make_uint4(w[0], w[1], w[2], w[3]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        unsigned o = __shfl_xor(mx, off, 64);
        mx = o > mx ? o : mx;
    }
    if ((tid & 63) == 0 && maxabs_bits) max_word(maxabs_bits, mx);
}

// order: 0 = 32x32x16 operands, 1 = 16x16x32 operands; f16: pts are fp16 bit patterns (order 1, kt = 128 / 256)
static int launch_prep_image_bf16(int order, int kt, int k, int npts, int npts_pad, const uint16_t *pts, float scale,
                                  float pad_norm, void *img, float *norms, unsigned *max_norm_bits, unsigned *maxabs_bits,
                                  hipStream_t st, bool f16)
{
    if (f16) {   // fp16 points: the order-1 image at the depths of the 16x16x32 tiles
        if (order == 1 && kt == 256)
            hipLaunchKernelGGL((image_bf16_kernel<256, true>), dim3(npts_pad / 32), dim3(256), 0, st, order, k, npts, pts,
                               scale, pad_norm, (uint16_t *)img, norms, max_norm_bits, maxabs_bits);
        else if (order == 1 && kt == 128)
            hipLaunchKernelGGL((image_bf16_kernel<128, true>), dim3(npts_pad / 32), dim3(256), 0, st, order, k, npts, pts,
                               scale, pad_norm, (uint16_t *)img, norms, max_norm_bits, maxabs_bits);
        else {
            set_error("prep: unsupported fp16 tile K %d (order %d)", kt, order);
            return NNS_ERR_UNSUPPORTED;
        }
        NNS_HIP(hipGetLastError());
        return NNS_OK;
    }
    if (kt == 256)
        hipLaunchKernelGGL(image_bf16_kernel<256>, dim3(npts_pad / 32), dim3(256), 0, st, order, k, npts, pts, scale,
                           pad_norm, (uint16_t *)img, norms, max_norm_bits, maxabs_bits);
    else if (kt == 512)   // (either operand order)
        hipLaunchKernelGGL(image_bf16_kernel<512>, dim3(npts_pad / 32), dim3(256), 0, st, order, k, npts, pts, scale,
                           pad_norm, (uint16_t *)img, norms, max_norm_bits, maxabs_bits);
    else if (kt == 1024 && order == 0)
        hipLaunchKernelGGL((image_deep_kernel<1024, uint16_t>), dim3(npts_pad / 32), dim3(256), 0, st, k, npts, pts,
                           (const float *)nullptr, scale, pad_norm, (uint16_t *)img, norms, max_norm_bits, maxabs_bits);
    else if (kt == 384 && order == 0)
        hipLaunchKernelGGL((image_deep_kernel<384, uint16_t, 128>), dim3(npts_pad / 32), dim3(256), 0, st, k, npts, pts,
                           (const float *)nullptr, scale, pad_norm, (uint16_t *)img, norms, max_norm_bits, maxabs_bits);
    else if (kt == 640 && order == 0)
        hipLaunchKernelGGL((image_deep_kernel<640, uint16_t, 128>), dim3(npts_pad / 32), dim3(256), 0, st, k, npts, pts,
                           (const float *)nullptr, scale, pad_norm, (uint16_t *)img, norms, max_norm_bits, maxabs_bits);
    else if (kt == 768 && order == 0)
        hipLaunchKernelGGL((image_deep_kernel<768, uint16_t, 256>), dim3(npts_pad / 32), dim3(256), 0, st, k, npts, pts,
                           (const float *)nullptr, scale, pad_norm, (uint16_t *)img, norms, max_norm_bits, maxabs_bits);
    else if (kt == 128 && order == 1)
        hipLaunchKernelGGL(image_bf16_kernel<128>, dim3(npts_pad / 32), dim3(256), 0, st, order, k, npts, pts, scale,
                           pad_norm, (uint16_t *)img, norms, max_norm_bits, maxabs_bits);
    else {
        set_error("prep: unsupported bf16 tile K %d (order %d)", kt, order);
        return NNS_ERR_UNSUPPORTED;
    }
    NNS_HIP(hipGetLastError());
    return NNS_OK;
}

// ---- int8 image (the operands of v_mfma_i32_16x16x64_i8) -----------------------------------
// One workgroup = one block of 32 points at KT = 256: eight 1 KiB fragments, fragment 4 t + ks = 16-point tile t x k-step
// ks of 64 dims; lane l holds dims 64 ks + 16 (l >> 4) .. + 15 of point 16 t + (l & 15), one operand (4 VGPRs) per
// ds_read_b128.  The bytes, blocks and fragment order of the 128-deep order-1 bf16 image.  The image holds the VALUES
// (-2 v does not fit int8: the filter applies the factor), zero-padded to KT; the norms are exact integers <= 2^22,
// stored as fp32.  int8 has no NaN / INF / huge value: no max-|v| word.
// BIAS (uint8 points): every byte that exists is stored as u ^ 0x80, which read as int8 is u - 128; (q - 128) - (r - 128) =
// q - r, so scores and distances on the biased image are those of the uint8 values.  The padding (dims k .. KT - 1, rows
// past the last point) holds 0 AFTER the bias, in queries and refs alike, and the norm is the sum over the k real
// dimensions of (u - 128)^2 <= 256 * 128^2 = 2^22.
template <int KT, bool BIAS>
__global__ __launch_bounds__(256) void image_i8_kernel(int k, int npts, const int8_t *__restrict__ pts, float pad_norm,
                                                       uint4 *__restrict__ img, float *__restrict__ norms,
                                                       unsigned *__restrict__ max_norm_bits)
{
    constexpr int LD = KT + 16, NKS = KT / 64;   // (rows stay 16-byte aligned)
    __shared__ __attribute__((aligned(16))) int8_t tile[32 * LD];
    const int tid = threadIdx.x;
    const int blk = blockIdx.x;
    const int p0 = blk * 32;
    constexpr unsigned FLIP = BIAS ? 0x80808080u : 0u;   // the top bit of each byte
    if ((k & 15) == 0 && (((uintptr_t)pts) & 15) == 0) {
        // sixteen values per load, only the chunks that exist: the block's rows are one contiguous run of 32 k bytes
        const int kc = k >> 4, nrows = min(32, npts - p0);
        const uint4 *src = reinterpret_cast<const uint4 *>(pts + (size_t)p0 * k);
        for (int e = tid; e < nrows * kc; e += 256) {
            const int i = e / kc, c = e - i * kc;
            uint4 v = src[e];
            if constexpr (BIAS) v = make_uint4(v.x ^ FLIP, v.y ^ FLIP, v.z ^ FLIP, v.w ^ FLIP);
            *reinterpret_cast<uint4 *>(&tile[i * LD + 16 * c]) = v;
        }
        for (int e = tid; e < 32 * (KT / 16); e += 256) {   // zero padding: dims k .. KT - 1, rows past the last point
            const int i = e / (KT / 16), c = e - i * (KT / 16);
            if (c >= kc || i >= nrows) *reinterpret_cast<uint4 *>(&tile[i * LD + 16 * c]) = make_uint4(0u, 0u, 0u, 0u);
        }
    } else if ((k & 3) == 0 && (((uintptr_t)pts) & 3) == 0) {
        for (int e = tid; e < 32 * (KT / 4); e += 256) {   // four values per load
            const int i = e / (KT / 4), t4 = e - i * (KT / 4);
            unsigned v = 0;
            if (4 * t4 < k && p0 + i < npts) v = *reinterpret_cast<const unsigned *>(pts + (size_t)(p0 + i) * k + 4 * t4) ^ FLIP;
            *reinterpret_cast<unsigned *>(&tile[i * LD + 4 * t4]) = v;
        }
    } else {
        for (int e = tid; e < 32 * KT; e += 256) {
            const int i = e / KT, t = e - i * KT;
            int8_t v = 0;
            if (t < k && p0 + i < npts) v = (int8_t)(pts[(size_t)(p0 + i) * k + t] ^ (int8_t)(FLIP & 0xFFu));
            tile[i * LD + t] = v;
        }
    }
    __syncthreads();
    {
        // point i = tid >> 3: eight lanes, 32 values each (KT / 4 words strided by 8), summed in int32
        const int i = tid >> 3, part = tid & 7;
        int acc = 0;
        for (int t4 = part; t4 < KT / 4; t4 += 8) {
            const unsigned w = *reinterpret_cast<const unsigned *>(&tile[i * LD + 4 * t4]);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int v = (int)(w << (24 - 8 * b)) >> 24;
                acc += v * v;
            }
        }
#pragma unroll
        for (int off = 4; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
        float nv = (float)acc;   // <= 256 * 128^2 = 2^22: exact
        unsigned nb = 0;
        if (p0 + i >= npts) nv = pad_norm;
        else nb = __float_as_uint(nv);
        if (part == 0) norms[p0 + i] = nv;
        if (max_norm_bits) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned o = __shfl_xor(nb, off, 64);
                nb = o > nb ? o : nb;
            }
            if ((tid & 63) == 0) max_word(max_norm_bits, nb);
        }
    }
    uint4 *out = img + (size_t)blk * (32 * KT / 16);
    for (int f = tid; f < (32 * KT / 16); f += 256) {
        const int s = f >> 6, lane = f & 63;
        const int t = s / NKS, ks = s % NKS;
        out[f] = *reinterpret_cast<const uint4 *>(&tile[(16 * t + (lane & 15)) * LD + 64 * ks + 16 * (lane >> 4)]);
    }
}

// bias (uint8 points): the image byte is u ^ 0x80, read as int8 u - 128; the padded dimensions hold 0 AFTER the bias
static int launch_prep_image_i8(int kt, int k, int npts, int npts_pad, const int8_t *pts, float pad_norm, void *img,
                                float *norms, unsigned *max_norm_bits, hipStream_t st, bool bias)
{
    if (kt != 256 || k > kt) {
        set_error("prep: unsupported int8 tile K %d (k = %d)", kt, k);
        return NNS_ERR_UNSUPPORTED;
    }
    if (bias)   // (uint8 points: the same bytes with the top bit flipped)
        hipLaunchKernelGGL((image_i8_kernel<256, true>), dim3(npts_pad / 32), dim3(256), 0, st, k, npts, pts, pad_norm,
                           (uint4 *)img, norms, max_norm_bits);
    else
        hipLaunchKernelGGL((image_i8_kernel<256, false>), dim3(npts_pad / 32), dim3(256), 0, st, k, npts, pts, pad_norm,
                           (uint4 *)img, norms, max_norm_bits);
    NNS_HIP(hipGetLastError());
    return NNS_OK;
}

// K2 on the refs or the queries of geometry g (nns_internal.h: what each side writes)
int launch_prep_points(const FilterGeom &g, PrepSide side, const PrepPoints &a, hipStream_t st)
{
    const bool refs = side == PREP_REFS;
    const FilterForm &f = kFilterForms[g.form];
    const int pad = refs ? g.n_pad : g.m_pad;
    const float scale = refs ? -2.0f : 1.0f, pad_norm = refs ? INFINITY : 0.0f;
    unsigned *const max_norm = refs ? &a.scal->ymax2_bits : nullptr;
    if (f.k2_image == K2_I8)
        return launch_prep_image_i8(g.kt, a.k, a.npts, pad, (const int8_t *)a.pts, pad_norm, a.img, a.norms, max_norm, st,
                                    g.dtype == DT_U8);
    // (the image order follows the tile: 16x16 tiles read order 1 = kBf16ImageOrder, which is every geometry the flag
    //  passes accept, so their K2 on the queries is the 1-NN search's)
    if (f.k2_image == K2_BF16)
        return launch_prep_image_bf16(g.lpq == 4 ? 1 : 0, g.kt, a.k, a.npts, pad, (const uint16_t *)a.pts, scale, pad_norm, a.img,
                                      a.norms, max_norm, refs ? &a.scal->r_maxabs_bits : &a.scal->q_maxabs_bits, st,
                                      g.form == FORM_F16);
    I8PreArgs pre{};
    if (a.i8pre) {
        const I8PreLayout lay = i8pre_layout(g, pad, refs);
        pre.img8 = (uint4 *)((char *)a.img + lay.img8);
        if (refs) pre.seeds = (int *)((char *)a.img + lay.aux);
        else pre.bound = (float *)((char *)a.img + lay.aux);
        pre.scal = a.scal;
    }
    return launch_prep_image(a.k, g.kt, a.npts, pad, (const float *)a.pts, a.mean, scale, pad_norm, (float *)a.img, a.norms,
                             max_norm, refs ? nullptr : &a.scal->q_maxabs_bits, st, refs && g.lazy_img ? 3 : f.k2_form,
                             a.i8pre ? &pre : nullptr);
}

// ---- SoA -> AoS (NNS_REFS_SOA) --------------------------------------------------------------
// Tile = 32 dims x 64 points through LDS: reads are 64 consecutive points of one dimension row
// (256 B / 128 B runs), writes 32 consecutive dims of one point (128 B / 64 B runs).  HBM-bound:
// 2 * n * k * esz bytes.  (The reference's mat_inv_kernel, core.cu:293-306, goes the other way
// with one thread per element and strided writes.)
template <typename T>
__global__ __launch_bounds__(256) void soa_to_aos_kernel(int k, int n, const T *__restrict__ src, T *__restrict__ dst)
{
    __shared__ T tile[32][64 + 2];
    const int j0 = blockIdx.x * 64, t0 = blockIdx.y * 32;
    for (int e = threadIdx.x; e < 32 * 64; e += 256) {
        const int t = e >> 6, j = e & 63;
        if (t0 + t < k && j0 + j < n) tile[t][j] = src[(size_t)(t0 + t) * n + j0 + j];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 64 * 32; e += 256) {
        const int j = e >> 5, t = e & 31;
        if (t0 + t < k && j0 + j < n) dst[(size_t)(j0 + j) * k + t0 + t] = tile[t][j];
    }
}

int launch_soa_to_aos(int k, int n, const void *src, void *dst, int esz, hipStream_t st)
{
    const dim3 grid(divup(n, 64), divup(k, 32));
    if (esz == 4)
        hipLaunchKernelGGL(soa_to_aos_kernel<float>, grid, dim3(256), 0, st, k, n, (const float *)src, (float *)dst);
    else
        hipLaunchKernelGGL(soa_to_aos_kernel<uint16_t>, grid, dim3(256), 0, st, k, n, (const uint16_t *)src,
                           (uint16_t *)dst);
    NNS_HIP(hipGetLastError());
    return NNS_OK;
}

}  // namespace nns
