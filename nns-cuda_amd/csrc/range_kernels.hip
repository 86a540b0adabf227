// range_kernels.hip — K7: exact fixed-radius neighbour search.  Every ref whose V0 distance to a query is at most
// radius2 (fp32, inclusive; NaN and +INF distances never), returned in CSR form: lims[m + 1] (int64) and the hits of
// query i at idx[lims[i] .. lims[i + 1]) in ascending index order, with their V0 distances.
//
// Scan: K6's geometry (lane = ref, a tile of QT queries in LDS read by broadcast, every (lane, query) pair one
// t-ascending V0 chain), instantiated twice over one per-pair loop:
//   count: a wave __ballot of the hit predicate per query and a popcount; the workgroup's total per query goes to
//          lims[i + 1] (one ref chunk) or to the workspace [m][chunks];
//   fill:  the same ballots; the four waves of a round exchange their popcounts through LDS (one barrier per round),
//          and a hit's slot is chunk start + hits of the earlier rounds + hits of the lower waves of this round + the
//          hits of the lower lanes of its wave (mbcnt).  Rounds, waves and lanes run through the chunk in ascending
//          ref order, so every position comes from counts: the output is index-ordered and deterministic.
// Between the two: one wave per query turns its chunk counts into exclusive offsets (several chunks) and a three-step
// scan (tile sums, one workgroup over the tile sums, tile scans) turns the query counts into lims, in 64 bits.
#include "nns_internal.h"

namespace nns {

constexpr int kRangeThreads = 256;
constexpr int kRangeWaves = kRangeThreads / 64;
constexpr int kRangeMinPerChunk = 1024;                // refs a chunk sees at least (its query tile load amortises)
constexpr int kRangeMaxGridX = 1 << 20;                // query groups per grid row (2^28 lanes; the limit is 2^32)
constexpr int kScanItems = 16;
constexpr int kScanTile = kRangeThreads * kScanItems;  // query counts per tile of the lims scan

// grid = query groups (x, continued in z: one grid dimension holds at most 2^32 lanes) x ref chunks (y).  offs:
// [m][chunks] (several chunks only): count writes the chunk's hit count, fill reads the chunk's start offset within
// the query's segment.  lims: count writes lims[i + 1] (one chunk only), fill reads lims[i].  idx / dist (fill): a
// null buffer is not written (a caller's zero-size allocation when there are no hits).
template <int QT, int VEC, typename T, bool FILL>
__global__ __launch_bounds__(kRangeThreads) void range_scan_kernel(int k, int m, int n, int per, int chunks,
                                                                   float radius2, const T *__restrict__ q,
                                                                   const T *__restrict__ r, int64_t index_base,
                                                                   int64_t *__restrict__ lims, int *__restrict__ offs,
                                                                   int *__restrict__ idx, float *__restrict__ dist)
{
    extern __shared__ __attribute__((aligned(16))) float rg_smem[];   // the fp32 query tile [QT][k]
    __shared__ int wcnt[2][kRangeWaves][QT];                          // per-wave hit counts (fill: ping-pong rounds)
    __shared__ int64_t start[QT];                                     // fill: slot of the chunk's first hit per query
    __shared__ int64_t stop[QT];                                      // fill: end of the query's segment
    float *sq = rg_smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = (int)(((int64_t)blockIdx.z * gridDim.x + blockIdx.x) * QT);
    if (q0 >= m) return;   // (the last z row's spare groups: the whole workgroup, before any barrier)
    const int c = blockIdx.y;
    const int j0 = (int)((int64_t)c * per);
    const int j1 = (int64_t)j0 + per < n ? j0 + per : n;

    load_query_tile<QT, kRangeThreads>(sq, q, q0, m, k);
    if (FILL && tid < QT) {
        const bool live = q0 + tid < m;
        start[tid] = live ? lims[q0 + tid] + (chunks > 1 ? offs[(size_t)(q0 + tid) * chunks + c] : 0) : 0;
        stop[tid] = live ? lims[q0 + tid + 1] : 0;
    }
    int run[QT];   // hits so far: of this wave (count), of the workgroup (fill; at most per)
#pragma unroll
    for (int u = 0; u < QT; ++u) run[u] = 0;
    __syncthreads();

    const int rounds = (j1 - j0 + kRangeThreads - 1) / kRangeThreads;
    int buf = 0;
    for (int rd = 0; rd < rounds; ++rd) {
        const int j = j0 + rd * kRangeThreads + tid;
        float sum[QT];
#pragma unroll
        for (int u = 0; u < QT; ++u) sum[u] = __builtin_nanf("");   // a lane past the chunk's end hits nothing
        if (j < j1) v0_lane_chains<QT, VEC, kLaneScanUnroll<QT>>(k, sq, r + (size_t)j * k, sum);
        // (every lane of the workgroup reaches the ballots: the round count is workgroup-uniform)
        unsigned hits = 0;   // bit u: this lane's ref is a hit of query u
#pragma unroll
        for (int u = 0; u < QT; ++u) {
            const bool hit = q0 + u < m && range_hit(sum[u], radius2);
            const int cnt = __popcll(__ballot(hit));
            hits |= (unsigned)hit << u;
            if (FILL) {
                if (lane == 0) wcnt[buf][wave][u] = cnt;
            } else {
                run[u] += cnt;
            }
        }
        if (!FILL) continue;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < QT; ++u) {
            int below = 0, all = 0;
#pragma unroll
            for (int w = 0; w < kRangeWaves; ++w) {
                const int cnt = wcnt[buf][w][u];
                below += w < wave ? cnt : 0;
                all += cnt;
            }
            const uint64_t mask = __ballot((hits >> u) & 1);   // (ballot again: cheaper than keeping QT masks live)
            const int64_t slot = start[u] + run[u] + below + lanes_below(mask);
            // (slot < stop holds whenever the refs and queries are those the count saw; the bound keeps a fill
            //  after the caller changed them inside the buffers)
            if (((hits >> u) & 1) && slot < stop[u]) {
                if (idx) idx[slot] = (int)(index_base + j);
                if (dist) dist[slot] = sum[u];
            }
            run[u] += all;
        }
        buf ^= 1;   // (a wave writes this half again only after every wave has passed the next round's barrier)
    }
    if (FILL) return;

    if (lane == 0) {
#pragma unroll
        for (int u = 0; u < QT; ++u) wcnt[0][wave][u] = run[u];
    }
    __syncthreads();
    if (tid < QT && q0 + tid < m) {
        int cnt = 0;
#pragma unroll
        for (int w = 0; w < kRangeWaves; ++w) cnt += wcnt[0][w][tid];
        if (chunks > 1) offs[(size_t)(q0 + tid) * chunks + c] = cnt;
        else lims[q0 + tid + 1] = cnt;
    }
}

// several chunks: per query, the chunk counts offs[i][0 .. chunks) -> exclusive offsets in place, their sum (at most n)
// -> lims[i + 1].  One wave per query, 64 chunks per step.
__global__ __launch_bounds__(kRangeThreads) void range_chunk_offsets_kernel(int *__restrict__ offs, int m, int chunks,
                                                                            int64_t *__restrict__ lims)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * kRangeWaves + (threadIdx.x >> 6);
    if (i >= m) return;   // (whole waves)
    int *row = offs + i * chunks;
    int carry = 0;
    for (int c0 = 0; c0 < chunks; c0 += 64) {
        const int c = c0 + lane;
        const int v = c < chunks ? row[c] : 0;
        int incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        if (c < chunks) row[c] = carry + incl - v;
        carry += __shfl(incl, 63);
    }
    if (lane == 0) lims[i + 1] = carry;
}

// exclusive scan of one value per thread over the workgroup; *total = the sum of all
__device__ int64_t block_exclusive_scan(int64_t v, int64_t *sh, int64_t *total)
{
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int d = 1; d < kRangeThreads; d <<= 1) {
        const int64_t o = tid >= d ? sh[tid - d] : 0;
        __syncthreads();
        sh[tid] += o;
        __syncthreads();
    }
    const int64_t incl = sh[tid];
    *total = sh[kRangeThreads - 1];
    __syncthreads();   // (sh is reused by the next call)
    return incl - v;
}

// lims[1 .. m] hold the query counts: sums[t] = the sum of tile t's kScanTile counts
__global__ __launch_bounds__(kRangeThreads) void range_tile_sums_kernel(const int64_t *__restrict__ lims, int m,
                                                                        int64_t *__restrict__ sums)
{
    __shared__ int64_t sh[kRangeThreads];
    const int64_t i0 = (int64_t)blockIdx.x * kScanTile + threadIdx.x * kScanItems;
    int64_t v = 0;
    for (int e = 0; e < kScanItems; ++e)
        if (i0 + e < m) v += lims[1 + i0 + e];
    int64_t total = 0;
    (void)block_exclusive_scan(v, sh, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: sums[0 .. tiles) -> exclusive prefix sums, in place
__global__ __launch_bounds__(kRangeThreads) void range_sums_scan_kernel(int64_t *__restrict__ sums, int tiles)
{
    __shared__ int64_t sh[kRangeThreads];
    int64_t carry = 0;
    for (int64_t t0 = 0; t0 < tiles; t0 += kScanTile) {
        const int64_t i0 = t0 + threadIdx.x * kScanItems;
        int64_t loc[kScanItems];
        int64_t v = 0;
        for (int e = 0; e < kScanItems; ++e) {
            loc[e] = i0 + e < tiles ? sums[i0 + e] : 0;
            v += loc[e];
        }
        int64_t total = 0;
        int64_t ex = carry + block_exclusive_scan(v, sh, &total);
        for (int e = 0; e < kScanItems; ++e) {
            if (i0 + e < tiles) sums[i0 + e] = ex;
            ex += loc[e];
        }
        carry += total;
    }
}

// lims[1 .. m]: query counts -> inclusive prefix sums plus the tile's offset (sums: null with one tile); lims[0] = 0
__global__ __launch_bounds__(kRangeThreads) void range_tile_scan_kernel(int64_t *__restrict__ lims, int m,
                                                                        const int64_t *__restrict__ sums)
{
    __shared__ int64_t sh[kRangeThreads];
    const int64_t i0 = (int64_t)blockIdx.x * kScanTile + threadIdx.x * kScanItems;
    int64_t loc[kScanItems];
    int64_t v = 0;
    for (int e = 0; e < kScanItems; ++e) {
        loc[e] = i0 + e < m ? lims[1 + i0 + e] : 0;
        v += loc[e];
    }
    int64_t total = 0;
    int64_t acc = (sums ? sums[blockIdx.x] : 0) + block_exclusive_scan(v, sh, &total);
    for (int e = 0; e < kScanItems; ++e) {
        acc += loc[e];
        if (i0 + e < m) lims[1 + i0 + e] = acc;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) lims[0] = 0;
}

// ---- host side ---------------------------------------------------------------------------------------------------
// workspace layout: the per-(query, chunk) counts / offsets [m][chunks] int32 (several chunks), then the tile sums
// int64 [tiles] (several tiles)
static size_t range_offs_bytes(const RangePlan &p, int m)
{
    return p.chunks > 1 ? ((size_t)m * p.chunks * sizeof(int) + 7) & ~(size_t)7 : 0;
}

int range_plan(int k, int m, int n, RangePlan *p)
{
    if (k <= 0 || m <= 0 || n <= 0) return NNS_ERR_INVALID;
    if ((size_t)k * sizeof(float) > 64 * 1024) {
        set_error("range search: k = %d exceeds the LDS query tile (k <= 16384)", k);
        return NNS_ERR_UNSUPPORTED;
    }
    // query-tile width: 16 queries; ref chunks worth their query tile
    const int tiles = divup(m, kScanTile);
    const size_t sums_bytes = tiles > 1 ? (size_t)tiles * sizeof(int64_t) : 0;
    const LaneScanGrid g = lane_scan_grid(k, m, n, 16, 0, 0, kRangeMinPerChunk, (size_t)m * sizeof(int),
                                          kWsBudget - sums_bytes);
    p->qt = g.qt;
    p->qgroups = g.qgroups;
    p->chunks = g.splits;
    p->per = g.per;
    // (the query tile, then the static per-wave counts and the fill's segment starts / ends)
    p->lds = (int)((size_t)g.qt * k * sizeof(float) + 2 * kRangeWaves * g.qt * sizeof(int) + 2 * g.qt * sizeof(int64_t));
    p->tiles = tiles;
    p->ws_bytes = range_offs_bytes(*p, m) + sums_bytes;
    return NNS_OK;
}

int range_scan_tiles(int m) { return divup(m, kScanTile); }

int launch_range_lims(int m, int chunks, int tiles, int *offs, int64_t *sums, int64_t *lims, hipStream_t st)
{
    if (chunks > 1) {
        hipLaunchKernelGGL(range_chunk_offsets_kernel, dim3(divup(m, kRangeWaves)), dim3(kRangeThreads), 0, st, offs, m,
                           chunks, lims);
        NNS_HIP(hipGetLastError());
    }
    if (tiles > 1) {
        hipLaunchKernelGGL(range_tile_sums_kernel, dim3(tiles), dim3(kRangeThreads), 0, st, lims, m, sums);
        NNS_HIP(hipGetLastError());
        hipLaunchKernelGGL(range_sums_scan_kernel, dim3(1), dim3(kRangeThreads), 0, st, sums, tiles);
        NNS_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(range_tile_scan_kernel, dim3(tiles), dim3(kRangeThreads), 0, st, lims, m, (const int64_t *)sums);
    NNS_HIP(hipGetLastError());
    return NNS_OK;
}

template <bool FILL, typename T>
static int launch_range_scan(const RangePlan &p, int k, int m, int n, const void *q, const void *r, float radius2,
                             int64_t base, int64_t *lims, int *offs, int *idx, float *dist, hipStream_t st)
{
    const T *qt = (const T *)q, *rt = (const T *)r;
    const bool vec = (k % 4 == 0) && (((uintptr_t)r & (4 * sizeof(T) - 1)) == 0);
    const unsigned gx = p.qgroups < kRangeMaxGridX ? p.qgroups : kRangeMaxGridX;
    const unsigned gz = (unsigned)divup(p.qgroups, (int)gx);
    return with_qt<16, 8, 4, 2, 1>(p.qt, [&](auto qtc) {
        constexpr int QT = decltype(qtc)::value;
        return launch_lds(vec ? range_scan_kernel<QT, 4, T, FILL> : range_scan_kernel<QT, 1, T, FILL>,
                          dim3(gx, p.chunks, gz), dim3(kRangeThreads), (size_t)QT * k * sizeof(float), st, k, m, n,
                          p.per, p.chunks, radius2, qt, rt, base, lims, offs, idx, dist);
    });
}

int launch_range_count(const RangePlan &p, int k, int m, int n, const void *q, const void *r, int dtype, float radius2,
                       int64_t *lims, void *ws, hipStream_t st)
{
    int *offs = p.chunks > 1 ? (int *)ws : nullptr;
    int64_t *sums = p.tiles > 1 ? (int64_t *)((char *)ws + range_offs_bytes(p, m)) : nullptr;
    NNS_TRY(with_point_type(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        return launch_range_scan<false, T>(p, k, m, n, q, r, radius2, 0, lims, offs, nullptr, nullptr, st);
    }));
    return launch_range_lims(m, p.chunks, p.tiles, offs, sums, lims, st);
}

int launch_range_fill(const RangePlan &p, int k, int m, int n, const void *q, const void *r, int dtype, float radius2,
                      int64_t base, const int64_t *lims, const void *ws, int *idx, float *dist, hipStream_t st)
{
    int *offs = p.chunks > 1 ? (int *)ws : nullptr;
    int64_t *l = const_cast<int64_t *>(lims);   // (read only by the fill instantiation)
    return with_point_type(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        return launch_range_scan<true, T>(p, k, m, n, q, r, radius2, base, l, offs, idx, dist, st);
    });
}

}  // namespace nns
