// topk_kernels.hip — K6: exact k-nearest-neighbour search (the kn nearest refs per query) with V0's arithmetic,
// and the top-K key utilities (merge of two sorted rows, unpack).
//
// K6 scan: lane = ref, a tile of QT queries in LDS read by broadcast (K1b's geometry), each (lane, query) pair one
// t-ascending V0 chain (v0_step).  Every query owns, in LDS, a sorted list of its kn best packed keys so far and a
// candidate queue; its threshold (the list's kn-th key, NNS_KEY_NONE while the list fills) is held in registers by
// every lane.  A lane whose key is below the threshold appends it to the query's queue (LDS atomic counter).  At the
// end of every round (one ref per lane) the workgroup flushes when some queue holds more than half its capacity
// (so the next round, at most 256 appends per query, cannot overflow it) and after the last round: the queues are
// sorted (bitonic, in LDS), merged into the lists by rank, and the thresholds lowered.  With random data appends
// become rare after the first rounds (about kn ln(refs / kn) per query and split), so the scan costs about what the
// 1-NN scan does per pair.  Keys are unique within a search (distinct indices), so integer order of the keys is
// (distance, index) order and every merge below is exact.
//
// grid = query groups x ref splits.  One split: the lists are the answer.  Several: every (group, split) writes its
// sorted list to a workspace [splits][m][kn] and topk_merge_splits_kernel ranks every entry among all the splits'
// entries of its query (binary searches in the sorted rows) and scatters the kn smallest into place.
#include "nns_internal.h"

namespace nns {

constexpr size_t kTopkLdsMax = 160 * 1024;
constexpr int kTopkMinPerSplit = 2048;             // refs a split sees at least (so that its list warm-up amortises)

static size_t topk_lds_bytes(int qt, int k, int kn)
{
    const size_t keys = (size_t)qt * (2 * kn + kTopkQueue) * sizeof(nns_key);
    return ((keys + 15) & ~(size_t)15) + (size_t)qt * k * sizeof(float);
}

// LDS: list[2][QT][kn] (ping-pong), queue[QT][kTopkQueue], then the fp32 query tile [QT][k]
// bstride: the scan's ref j is row (j / 32) * bstride * 32 + j % 32 of r — every bstride-th 32-ref block (K6m's sample,
// topk_mfma.hip; n then counts the sampled refs).  1: r's rows as they are.
template <int QT, int VEC, typename T>
__global__ __launch_bounds__(kTopkThreads) void topk_scan_kernel(int k, int m, int n, int per, int kn, int bstride,
                                                                 const T *__restrict__ q, const T *__restrict__ r,
                                                                 int64_t index_base, nns_key *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) nns_key tk_smem[];
    __shared__ int qcnt[QT];
    nns_key *lists = tk_smem;                              // [2][QT][kn]
    nns_key *queue = tk_smem + 2 * QT * kn;                // [QT][kTopkQueue]
    const size_t key_bytes = (size_t)QT * (2 * kn + kTopkQueue) * sizeof(nns_key);
    float *sq = reinterpret_cast<float *>(reinterpret_cast<char *>(tk_smem) + ((key_bytes + 15) & ~(size_t)15));
    const int tid = threadIdx.x;
    const int q0 = blockIdx.x * QT;
    const int j0 = blockIdx.y * per;
    const int j1 = (int64_t)j0 + per < n ? j0 + per : n;

    load_query_tile<QT, kTopkThreads>(sq, q, q0, m, k);
    for (int e = tid; e < 2 * QT * kn; e += kTopkThreads) lists[e] = NNS_KEY_NONE;
    if (tid < QT) qcnt[tid] = 0;
    __syncthreads();

    int cur = 0;   // which half of the ping-pong lists holds the current lists
    nns_key thr[QT];
#pragma unroll
    for (int u = 0; u < QT; ++u) thr[u] = NNS_KEY_NONE;
    const int rounds = (j1 - j0 + kTopkThreads - 1) / kTopkThreads;
    for (int rd = 0; rd < rounds; ++rd) {
        const int j = j0 + rd * kTopkThreads + tid;
        int near_full = 0;
        if (j < j1) {
            float sum[QT];
            const int jr = bstride == 1 ? j : ((j >> 5) * bstride << 5) + (j & 31);
            v0_lane_chains<QT, VEC, kLaneScanUnroll<QT>>(k, sq, r + (size_t)jr * k, sum);
#pragma unroll
            for (int u = 0; u < QT; ++u) {
                const nns_key key = make_key(sum[u], index_base + jr);   // NaN / +INF -> NNS_KEY_NONE: never below thr
                if (key < thr[u]) {
                    const int pos = atomicAdd(&qcnt[u], 1);
                    queue[u * kTopkQueue + pos] = key;
                    near_full |= pos >= kTopkFlushAt;
                }
            }
        }
        // (the lane whose append crossed the mark knows it: one barrier decides for the whole workgroup)
        const bool flush = __syncthreads_or(near_full) || rd == rounds - 1;
        if (!flush) continue;

        topk_flush<QT>(lists, queue, qcnt, kn, cur, thr);
    }

    const nns_key *fin = lists + cur * QT * kn;
    for (int e = tid; e < QT * kn; e += kTopkThreads) {
        const int u = e / kn, i = e - u * kn;
        if (q0 + u < m) out[((size_t)blockIdx.y * m + q0 + u) * kn + i] = fin[e];
    }
}

// grid (query, split): entry i of split s's row goes to rank i + #(entries of lower splits <= it) + #(entries of
// higher splits < it) — a stable merge, so equal keys (none within one search) would still land in distinct slots
__global__ __launch_bounds__(kTopkThreads) void topk_merge_splits_kernel(const nns_key *__restrict__ ws, int m, int kn,
                                                                         int splits, nns_key *__restrict__ out)
{
    const int qi = blockIdx.x, s = blockIdx.y, i = threadIdx.x;
    nns_key *orow = out + (size_t)qi * kn;
    if (s == 0) {
        // slots behind the last selectable entry hold NNS_KEY_NONE
        int total = 0;
        for (int s2 = 0; s2 < splits; ++s2) total += tk_rank(ws + ((size_t)s2 * m + qi) * kn, kn, NNS_KEY_NONE - 1, true);
        for (int p = total + i; p < kn; p += blockDim.x) orow[p] = NNS_KEY_NONE;
    }
    if (i >= kn) return;
    const nns_key v = ws[((size_t)s * m + qi) * kn + i];
    if (v == NNS_KEY_NONE) return;
    int rk = i;
    for (int s2 = 0; s2 < splits && rk < kn; ++s2)
        if (s2 != s) rk += tk_rank(ws + ((size_t)s2 * m + qi) * kn, kn, v, s2 < s);
    if (rk < kn) orow[rk] = v;
}

// nns_keys_topk_merge: one workgroup per row, both rows staged in LDS (the output overwrites `inout`)
__global__ __launch_bounds__(kTopkThreads) void topk_merge_pair_kernel(nns_key *__restrict__ inout,
                                                                       const nns_key *__restrict__ other, int kn)
{
    __shared__ nns_key a[NNS_TOPK_MAX];
    __shared__ nns_key b[NNS_TOPK_MAX];
    const size_t row = (size_t)blockIdx.x * kn;
    const int i = threadIdx.x;
    if (i < kn) {
        a[i] = inout[row + i];
        b[i] = other[row + i];
    }
    __syncthreads();
    if (i >= kn) return;
    const int na = tk_rank(a, kn, NNS_KEY_NONE - 1, true), nb = tk_rank(b, kn, NNS_KEY_NONE - 1, true);
    if (i >= na + nb) inout[row + i] = NNS_KEY_NONE;
    if (i < na) {
        const int rk = i + tk_rank(b, nb, a[i], false);
        if (rk < kn) inout[row + rk] = a[i];
    }
    if (i < nb) {
        const int rk = i + tk_rank(a, na, b[i], true);
        if (rk < kn) inout[row + rk] = b[i];
    }
}

__global__ void topk_unpack_kernel(const nns_key *__restrict__ keys, size_t count, int *__restrict__ idx,
                                   float *__restrict__ dist)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += stride) {
        const nns_key kx = keys[e];
        idx[e] = kx == NNS_KEY_NONE ? -1 : (int)(uint32_t)(kx & 0xFFFFFFFFull);
        if (dist) dist[e] = __uint_as_float((uint32_t)(kx >> 32));   // NNS_KEY_NONE -> +INF
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------
int topk_plan(int k, int m, int n, int kn, TopkPlan *p)
{
    if (k <= 0 || m <= 0 || n <= 0 || kn <= 0) return NNS_ERR_INVALID;
    if (kn > NNS_TOPK_MAX) {
        set_error("top-K: kn = %d above 256", kn);
        return NNS_ERR_UNSUPPORTED;
    }
    if ((size_t)k * sizeof(float) > 64 * 1024) {
        set_error("top-K: k = %d exceeds the LDS query tile (k <= 16384)", k);
        return NNS_ERR_UNSUPPORTED;
    }
    // query-tile width: 16 queries while the lists are short, 8 beyond; ref splits worth their list warm-up
    const LaneScanGrid g = lane_scan_grid(k, m, n, kn <= 16 ? 16 : 8, topk_lds_bytes(1, k, kn), kTopkLdsMax,
                                          kn * 16 > kTopkMinPerSplit ? kn * 16 : kTopkMinPerSplit,
                                          (size_t)m * kn * sizeof(nns_key), kWsBudget);
    p->qt = g.qt;
    p->qgroups = g.qgroups;
    p->splits = g.splits;
    p->per = g.per;
    p->lds = (int)(topk_lds_bytes(g.qt, k, kn) + g.qt * sizeof(int));
    p->ws_keys = g.splits > 1 ? (size_t)g.splits * m * kn : 0;
    return NNS_OK;
}

template <typename T>
static int launch_topk_scan(const TopkPlan &p, int k, int m, int n, int kn, int bstride, const T *q, const T *r,
                            int64_t base, nns_key *out, hipStream_t st)
{
    const bool vec = (k % 4 == 0) && (((uintptr_t)r & (4 * sizeof(T) - 1)) == 0);
    return with_qt<16, 8, 4, 2, 1>(p.qt, [&](auto qt) {
        constexpr int QT = decltype(qt)::value;
        return launch_lds(vec ? topk_scan_kernel<QT, 4, T> : topk_scan_kernel<QT, 1, T>, dim3(p.qgroups, p.splits),
                          dim3(kTopkThreads), topk_lds_bytes(QT, k, kn), st, k, m, n, p.per, kn, bstride, q, r, base, out);
    });
}

int launch_topk_search(const TopkPlan &p, int k, int m, int n, int kn, const void *q, const void *r, int dtype,
                       int64_t base, nns_key *keys, nns_key *ws, hipStream_t st, int bstride)
{
    nns_key *scan_out = p.splits > 1 ? ws : keys;
    NNS_TRY(with_point_type(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        return launch_topk_scan<T>(p, k, m, n, kn, bstride, (const T *)q, (const T *)r, base, scan_out, st);
    }));
    if (p.splits > 1) NNS_TRY(launch_topk_merge_splits(ws, m, m, kn, p.splits, keys, st));
    return NNS_OK;
}

int launch_topk_merge_splits(const nns_key *ws, int m, int rows, int kn, int splits, nns_key *keys, hipStream_t st)
{
    const int threads = (kn + 63) / 64 * 64;
    hipLaunchKernelGGL(topk_merge_splits_kernel, dim3(rows, splits), dim3(threads), 0, st, ws, m, kn, splits, keys);
    NNS_HIP(hipGetLastError());
    return NNS_OK;
}

int launch_topk_merge(nns_key *inout, const nns_key *other, int m, int kn, hipStream_t st)
{
    const int threads = (kn + 63) / 64 * 64;
    hipLaunchKernelGGL(topk_merge_pair_kernel, dim3(m), dim3(threads), 0, st, inout, other, kn);
    NNS_HIP(hipGetLastError());
    return NNS_OK;
}

int launch_topk_unpack(const nns_key *keys, int m, int kn, int *idx, float *dist, hipStream_t st)
{
    const size_t count = (size_t)m * kn;
    size_t blocks = (count + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(topk_unpack_kernel, dim3((unsigned)blocks), dim3(256), 0, st, keys, count, idx, dist);
    NNS_HIP(hipGetLastError());
    return NNS_OK;
}

}  // namespace nns
