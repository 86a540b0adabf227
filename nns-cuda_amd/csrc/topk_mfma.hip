// topk_mfma.hip — K6m: the MFMA-filtered top-K search (NNS_TOPK_MFMA; fp32 points on split-bf16 operands, bf16 points
// on exact operands: K7m's two flag kernels).
//
// K6 evaluates V0's distance for every (query, ref) pair.  K6m first finds, per query, a distance U that the kn-th
// nearest ref cannot exceed, asks the matrix cores which 32-ref blocks can hold a ref within U, and selects among those:
//   bound:   K6's own scan (topk_scan_kernel, block stride > 1) over every stride-th 32-ref block of the ORIGINAL points;
//            U_i = the kn-th smallest V0 distance of the sample (topk_bound_kernel reads it off the scan's rows, which
//            sit in the caller's key buffer until the selection overwrites them).  The kn-th smallest over a subset is
//            at least the kn-th smallest over all refs, so every ref among the true kn nearest has d0 <= U_i, ties at
//            the kn-th distance included.
//   flag:    K7m's flag pass (range_mfma.hip) with radius2 = U_i per query: every ref with d0 <= U_i has its block's bit
//            set (range_threshold's theorem).  A query whose bound is not finite (fewer than kn selectable sample refs)
//            or whose values void the filter's error model gets its row filled.
//   select:  one workgroup per (query, chunk of flag words) walks the words in ascending order; its eight half-waves
//            take the flagged blocks, lane = ref, V0's chain on the original points (v0_lane_chains).  A key below the
//            threshold is appended to the query's LDS queue; the threshold starts just above every key of distance U_i
//            and drops to the list's kn-th key after each flush (topk_flush, K6's).  Several chunks: the chunks' lists
//            go to the index's split workspace and topk_merge_splits_kernel merges them.
// The selection sees a superset of the true kn nearest and ranks it by V0's keys: the rows are K6's bit for bit, and a
// false flag costs time only.  DESIGN section 4, "K6m".
#include "nns_internal.h"

namespace nns {

constexpr int kTmStepBlocks = kRmChunkWords * 32;   // blocks of one step of flag words

// LDS of a selection workgroup: list[2][kn] (ping-pong), queue[kTopkQueue], the step's flagged blocks, the query [k]
static size_t topk_select_lds(int k, int kn)
{
    return (size_t)(2 * kn + kTopkQueue) * sizeof(nns_key) + (size_t)kTmStepBlocks * sizeof(int) + (size_t)k * sizeof(float);
}

__global__ void topk_bound_kernel(const nns_key *__restrict__ keys, int m, int kn, float *__restrict__ bound)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const nns_key kx = keys[(size_t)i * kn + kn - 1];
    bound[i] = __uint_as_float((uint32_t)(kx >> 32));   // NNS_KEY_NONE -> +INF
}

// grid = queries of the batch x chunks.  Query i = i0 + blockIdx.x (flag row blockIdx.x), flag words [c * per,
// min((c + 1) * per, wpq)); its sorted list goes to out[(c * m + i) * kn ...].
template <int VEC, typename T>
__global__ __launch_bounds__(kTopkThreads) void topk_select_kernel(int k, int i0, int m, int n, int kn, int per, int wpq,
                                                                   const T *__restrict__ q, const T *__restrict__ r,
                                                                   const unsigned *__restrict__ flags,
                                                                   const float *__restrict__ bound, int64_t index_base,
                                                                   nns_key *__restrict__ out,
                                                                   unsigned long long *__restrict__ stat)
{
    extern __shared__ __attribute__((aligned(16))) nns_key tm_smem[];
    __shared__ int qcnt[1];
    __shared__ int nlist;
    nns_key *lists = tm_smem;                  // [2][kn]
    nns_key *queue = tm_smem + 2 * kn;         // [kTopkQueue]
    int *blist = reinterpret_cast<int *>(queue + kTopkQueue);    // [kTmStepBlocks], 16-byte aligned (16 kn + 4096 bytes in)
    float *sq = reinterpret_cast<float *>(blist + kTmStepBlocks);
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t i = (int64_t)i0 + blockIdx.x;
    const int c = blockIdx.y;

    for (int t = tid; t < k; t += kTopkThreads) sq[t] = pt_ld1(q + (size_t)i * k + t);   // (widened to fp32)
    for (int e = tid; e < 2 * kn; e += kTopkThreads) lists[e] = NNS_KEY_NONE;
    if (tid == 0) qcnt[0] = 0;
    // d0 == U passes, anything above (a false flag's refs) does not; no finite bound: every selectable key passes
    const float u = bound[i];
    const nns_key thr0 = u < __builtin_inff() ? (nns_key)(__float_as_uint(u) + 1u) << 32 : (nns_key)NNS_KEY_NONE;
    nns_key thr[1] = {thr0};
    int cur = 0;
    const unsigned *frow = flags + (size_t)blockIdx.x * wpq;
    const int w0 = c * per, w1 = w0 + per < wpq ? w0 + per : wpq;
    const int nblk = (n + 31) >> 5;   // blocks that hold a ref
    unsigned flagged = 0;
    __syncthreads();

    for (int wb = w0; wb < w1; wb += kRmChunkWords) {
        if (tid < 64) {
            // the first wave lists the step's flagged blocks in ascending order (a scan of the words' bit counts)
            const int w = wb + lane;
            unsigned word = w < w1 ? frow[w] : 0u;
            // (bits of blocks past the refs — a filled row, padding blocks — are dropped)
            const int first = w << 5;
            if (first + 32 > nblk) word = first >= nblk ? 0u : word & (0xFFFFFFFFu >> (first + 32 - nblk));
            const int cnt = __popc(word);
            flagged += cnt;
            int incl = cnt;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int t = __shfl_up(incl, d);
                if (lane >= d) incl += t;
            }
            int pos = incl - cnt;
            while (word) {
                blist[pos++] = first + __builtin_ctz(word);
                word &= word - 1;
            }
            if (lane == 63) nlist = incl;
        }
        __syncthreads();
        const int nl = nlist;
        for (int it = 0; it < nl; it += kTopkThreads / 32) {   // one flagged block per half-wave and round
            const int e = it + (tid >> 5);
            int near_full = 0;
            if (e < nl) {
                const int64_t j = ((int64_t)blist[e] << 5) + (tid & 31);
                if (j < n) {
                    float sum[1];
                    v0_lane_chains<1, VEC, 8>(k, sq, r + (size_t)j * k, sum);
                    const nns_key key = make_key(sum[0], index_base + j);   // NaN / +INF -> NNS_KEY_NONE: never below thr
                    if (key < thr[0]) {
                        const int pos = atomicAdd(&qcnt[0], 1);
                        queue[pos] = key;
                        near_full = pos >= kTopkFlushAt;
                    }
                }
            }
            // (a round appends at most 256 keys: a queue flushed beyond kTopkFlushAt cannot overflow in the next one)
            if (__syncthreads_or(near_full)) {
                topk_flush<1>(lists, queue, qcnt, kn, cur, thr);
                if (thr[0] > thr0) thr[0] = thr0;   // (the list is not full yet)
            }
        }
        __syncthreads();   // the step's block list has been read by everyone before the next step rewrites it
    }
    topk_flush<1>(lists, queue, qcnt, kn, cur, thr);

    const nns_key *fin = lists + cur * kn;
    for (int e = tid; e < kn; e += kTopkThreads) out[((size_t)c * m + i) * kn + e] = fin[e];
    if (tid < 64) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) flagged += __shfl_xor((int)flagged, d);
        if (lane == 0 && flagged) atomicAdd(stat, (unsigned long long)flagged);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------
// The sample rule.  With S sample refs about kn n / S refs lie within the bound, each in a block of 32, so the selection
// evaluates about 32 kn n / S refs after the bound scan's S.  A selected ref costs w times a scanned one — the selection
// reads a ref row for ONE query where K6's scan shares it among the 8 or 16 queries of its tile; measured, w is about 1
// at k = 16 and about 20 at k = 128 ("K6m") — so S + w 32 kn n / S is least at S = sqrt(32 kn n w).
// With w = max(k, 16) / 16:  sb = max(ceil(sqrt(kn n max(k, 16) / 512)), ceil(max(2048, 16 kn) / 32)) blocks; the floor
// keeps the scan's list warm-up small against the sample.  Where that asks for more than every second block and the
// unweighted rule (w = 1) does not, every second block is taken.  Every floor(blocks / sb)-th block is taken, so the
// sample is spread over the whole ref range.
int topk_mfma_plan(int k, int m, int n, int kn, bool split_eager, TopkMfmaPlan *p, int dtype)
{
    const PointType &pt = point_type(dtype);
    const bool bf16 = dt_bf16_like(dtype);   // (bf16 and uint8 points: the depths of the 16x16 tiles)
    if (k <= 0 || m <= 0 || n <= 0 || kn <= 0) return NNS_ERR_INVALID;
    if (kn > NNS_TOPK_MAX) {
        set_error("top-K: kn = %d above 256", kn);
        return NNS_ERR_UNSUPPORTED;
    }
    if ((unsigned)dtype >= DT_COUNT || !pt.flag_kmax) {   // (no caller passes one: range_mfma_plan's refusal, made here too)
        set_error("the top-K MFMA flag: no flag pass for point dtype %d", dtype);
        return NNS_ERR_UNSUPPORTED;
    }
    if (k < pt.flag_kmin || k > pt.flag_kmax) {
        set_error(bf16 ? "the top-K MFMA flag: k = %d outside 32 .. 256 (bf16 and uint8 points: the 16x16 tiles)"
                       : "the top-K MFMA flag: k = %d outside 8 .. 256 (the split-bf16 tiles)", k);
        return NNS_ERR_UNSUPPORTED;
    }
    *p = TopkMfmaPlan{};
    const int blocks = divup(n, 32);
    const int64_t floor_blocks = divup(kn * 16 > 2048 ? kn * 16 : 2048, 32);
    const auto sample_blocks = [&](int64_t w16) {   // max(ceil(sqrt(kn n w16 / 512)), the floor)
        const int64_t knw = (int64_t)kn * n * w16;
        int64_t v = (int64_t)ceil(sqrt((double)knw / 512.0));
        while (v * v * 512 < knw) ++v;   // (the ceiling, whatever sqrt rounded to)
        return v > floor_blocks ? v : floor_blocks;
    };
    const int64_t sb0 = sample_blocks(16), half = blocks / 2;
    int64_t sb = sample_blocks(k > 16 ? k : 16);
    if (sb > half) sb = sb0 > half ? sb0 : half;
    p->stride = (int)(blocks / sb);
    const int step = p->stride > 1 ? p->stride : 1;
    p->sample_blocks = divup(blocks, step);
    const int64_t last = (int64_t)(p->sample_blocks - 1) * step * 32;   // the last sampled block's first ref, < n
    p->sample_refs = (int)((int64_t)(p->sample_blocks - 1) * 32 + (n - last < 32 ? n - last : 32));
    p->lds = (int)topk_select_lds(k, kn);
    if (p->stride < 2 || m < kTopkMfmaMinQueries) return NNS_OK;
    if (range_mfma_plan(k, m, n, split_eager, &p->rp, dtype) != NNS_OK) {
        p->rp = RangeMfmaPlan{};
        return NNS_OK;
    }
    NNS_TRY(topk_plan(k, m, p->sample_refs, kn, &p->sp));
    const size_t chunk_keys = p->rp.echunks > 1 ? (size_t)p->rp.echunks * m * kn : 0;
    p->ws_keys = chunk_keys > p->sp.ws_keys ? chunk_keys : p->sp.ws_keys;
    p->filtered = 1;
    return NNS_OK;
}

int launch_topk_bound(const nns_key *keys, int m, int kn, float *bound, hipStream_t st)
{
    hipLaunchKernelGGL(topk_bound_kernel, dim3(divup(m, 256)), dim3(256), 0, st, keys, m, kn, bound);
    NNS_HIP(hipGetLastError());
    return NNS_OK;
}

template <typename T>
static int launch_topk_select_t(const TopkMfmaPlan &p, int k, int i0, int rows, int m, int n, int kn, const T *q, const T *r,
                                const void *flags, const float *bound, int64_t base, nns_key *out,
                                unsigned long long *stat, hipStream_t st)
{
    // (K6's rule: four values of a row per load where the rows are 16- (fp32) / 8-byte (bf16) / 4-byte (uint8) aligned)
    const bool vec = (k % 4 == 0) && (((uintptr_t)r & (4 * sizeof(T) - 1)) == 0);
    return launch_lds(vec ? topk_select_kernel<4, T> : topk_select_kernel<1, T>, dim3(rows, p.rp.echunks), dim3(kTopkThreads),
                      topk_select_lds(k, kn), st, k, i0, m, n, kn, p.rp.eper, p.rp.wpq, q, r, (const unsigned *)flags, bound,
                      base, out, stat);
}

int launch_topk_select(const TopkMfmaPlan &p, int k, int i0, int rows, int m, int n, int kn, const void *q, const void *r,
                       const void *flags, const float *bound, int64_t base, nns_key *out, unsigned long long *stat,
                       hipStream_t st)
{
    if (p.rp.dtype == DT_U8)
        return launch_topk_select_t(p, k, i0, rows, m, n, kn, (const u8_t *)q, (const u8_t *)r, flags, bound, base, out, stat,
                                    st);
    if (p.rp.dtype == DT_BF16)
        return launch_topk_select_t(p, k, i0, rows, m, n, kn, (const uint16_t *)q, (const uint16_t *)r, flags, bound, base,
                                    out, stat, st);
    return launch_topk_select_t(p, k, i0, rows, m, n, kn, (const float *)q, (const float *)r, flags, bound, base, out, stat,
                                st);
}

}  // namespace nns
