/*
 * nns.h — C ABI of the MI355X-native brute-force nearest-neighbour engine.
 *
 * This is the drop-in boundary for the reference's "distance matrix + argmin"
 * path (sty-hhh/NNS-CUDA, V0-V9).  Every entry point is plain C: pointers and
 * sizes, no C++/torch types.  The shared library is libnns_mi355x.so
 * (nns-cuda_amd/csrc, hand-written HIP for gfx950).
 *
 * Reference interface replaced (file:line are into the reference tree):
 *   - vN::cudaCall(int k, int m, int n, float *s_points, float *r_points,
 *                  int **results)                     core.cu:23-29 (V0) and the
 *     identical signatures at core.cu:123, 177, 258, 350, 427, 538, 634, 761,
 *     965; selected through the function pointer of main.cu:7, called at
 *     main.cu:74.                                  -> nns_search_f32()
 *   - the per-GPU shard body of V8/V9 (core.cu:778-829, 982-1033): upload a
 *     contiguous ref shard, transpose (mat_inv_kernel core.cu:293-306), run the
 *     fused distance+argmin kernel.                -> nns_index_create() +
 *                                                     nns_index_search()
 *   - the V7/V8/V9 second-stage merge (core.cu:675-696, 832-852, 1036-1056).
 *                                                  -> nns_keys_min() /
 *                                                     an RCCL min all-reduce on
 *                                                     the packed keys.
 *   - utils.h CHECK (print + exit(1), utils.h:16-26): the C ABI never exits; it
 *     returns a status code (the C++ shim mi355x::cudaCall reproduces the
 *     print-and-exit behaviour, see nns_cudacall.hpp).
 *
 * Semantics (identical to the reference's V0, core.cu:31-52): for every query
 * i, the index j in [0,n) minimising the fp32 value
 *     sum_{t=0..k-1, t ascending} fl( fl(q[i][t] - r[j][t])^2 )
 * (un-contracted IEEE fp32, starting from 0), the LOWEST index winning exact
 * ties; a NaN or +INF distance is never selected; a row with no selectable
 * distance returns index 0.  Indices are bit-exact against V0; the returned
 * distance is that same fp32 value (bit-equal, tolerance 0 ulp).
 *
 * Layouts: queries s_points[m][k], refs r_points[n][k], row-major fp32
 * (core.cu:41); results int32[m], 0-based global ref index.
 *
 * Threading: one caller thread per nns_index, and searches of ONE index must not
 * overlap in time (its workspaces, incl. the exact kernel's merge accumulator, belong
 * to the index: use one index per stream).  The whole-call entry points are
 * re-entrant: the process-wide caches behind them (workspace pool, the small-call
 * scratch, RCCL communicators) are internally synchronised, and a call that finds the
 * scratch busy takes the plain path.  All device work of the split API is enqueued on
 * the caller's HIP stream and is asynchronous unless stated.
 *
 * Manners towards the host application:
 *   - no entry point calls hipDeviceSynchronize(): destroy, workspace regrow and the whole-call exits hand
 *     their device blocks back to the library's pool behind an EVENT on the stream that used them, read-outs
 *     (nns_index_stats, nns_index_near_ties) wait for the index's own stream, and the whole-call entry points
 *     run their kernels on a non-blocking stream of the library.  Kernels the application has running on
 *     other streams are never waited for by the library.  (The stream an index last worked on must still exist
 *     when the index is destroyed; if it does not, destroy falls back to waiting for the device.  The HIP runtime
 *     multiplexes streams onto a few hardware queues: work that lands on the queue of a long-running foreign kernel
 *     runs behind it whatever a library does.)
 *   - every entry point that selects a device restores the caller's current device before it returns.
 */
#ifndef NNS_MI355X_H
#define NNS_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NNS_VERSION_MAJOR 0
#define NNS_VERSION_MINOR 1

/* status codes */
enum {
    NNS_OK = 0,
    NNS_ERR_INVALID = 1,   /* bad argument (k,m,n <= 0, null pointer, ...) */
    NNS_ERR_HIP = 2,       /* a HIP runtime call failed: see nns_last_error() */
    NNS_ERR_NOMEM = 3,     /* host or device allocation failed */
    NNS_ERR_NODEVICE = 4,  /* no gfx950 device visible */
    NNS_ERR_UNSUPPORTED = 5
};

/* path selection flags (nns_index_create / nns_search_f32_ex) */
enum {
    NNS_PATH_AUTO = 0,   /* MFMA filter for 8 <= k <= 1024 (bf16 points: 32..1024) and >= 64 queries (small 8- / 16-D
                          * problems excepted), exact kernels otherwise */
    NNS_PATH_EXACT = 1,  /* exact per-pair kernels only (V1..V9 arithmetic re-expressed) */
    NNS_PATH_MFMA = 2,   /* -2*Q*R^T MFMA filter + exact re-rank (k padded to the tile K) */
    NNS_PATH_MASK = 3,
    NNS_PROFILE = 16,    /* record HIP-event timings per stage (adds syncs at read-out) */
    NNS_MULTI_VIRTUAL = 32, /* nns_search_f32_multi: allow more shards than GPUs (rehearsal) */
    NNS_FILTER_BF16 = 128, /* OPT-IN, fp32 points only, k <= 1024: run the MFMA filter on the centred points
                          * rounded to bf16 (v_mfma_f32_16x16x32_bf16: 16x the fp32 MFMA rate) with a margin tau
                          * widened by the rounding bound 2^-6 |x'||y'|, then re-rank the candidates with V0's fp32
                          * arithmetic on the ORIGINAL fp32 points as usual.  Indices and distances are the same
                          * bits as without the flag (the filter only decides which refs are re-ranked); queries
                          * whose candidate lists overflow fall back to the exact scan.  NNS_PATH_AUTO
                          * takes this filter by itself only for 256 < k <= 1024, where no fp32 tile exists (the
                          * alternative is the VALU scan); it is not what bench.py measures for the fp32
                          * configurations. */
    NNS_REFS_SOA = 64,   /* the reference points are given dimension-major, r[t * n + j] (a dense [k][n]
                          * array: the layout v4::mat_inv_kernel produces, core.cu:293-306, :327) instead
                          * of r[j * k + t]; queries stay [m][k].  The library transposes once on the
                          * device into a copy it owns. */
    NNS_RECORDS_PER_REF = 512, /* MFMA filter: keep the candidate records per SCORE (the form long reference streams
                          * use) also on short streams, where AUTO records ref TILES (a lane's two best tiles, or one
                          * record per tile within its threshold) and lets K5 evaluate the tile's rows — same results
                          * either way; lets tests and A/B runs drive both forms at any size */
    NNS_FILTER_F32 = 1024, /* MFMA filter, fp32 points: fp32 operands (v_mfma_f32_32x32x2_f32) instead of the default
                          * split-bf16 operands (each centred value as hi = rn_bf16(v) plus lo = rn_bf16(v - hi), the
                          * dot product as hi.hi + hi.lo + lo.hi on v_mfma_f32_32x32x16_bf16, 3/16 of the fp32 MFMA
                          * work, with tau widened by ~3 * 2^-15 |x'||y'|).  Same indices and distances either way;
                          * for A/B runs and tests of the fp32-operand filter.  With bf16 points or with
                          * NNS_FILTER_BF16: NNS_ERR_INVALID.  k > 256 has no fp32 tile: AUTO still takes the
                          * bf16-operand filter there, NNS_PATH_MFMA returns NNS_ERR_UNSUPPORTED */
    NNS_FILTER_SPLIT_EAGER = 2048, /* MFMA filter, fp32 points on split-bf16 operands: the EAGER schedule (all three
                          * products of every tile) and image layout at every depth, instead of the lazy schedule the
                          * library takes where it measured faster (KT = 128 on long streams: the two cross products only on
                          * tiles whose hi-hi minimum is within B of the lane's threshold).  Same candidate lists' meaning,
                          * same indices and distances; for A/B runs, tests, and data so tightly clustered that most tiles
                          * refine.  NNS_ERR_INVALID with bf16 points, NNS_FILTER_BF16 or NNS_FILTER_F32 */
    NNS_RANGE_MFMA = 4096, /* range search through the MFMA flag pass (K7m): nns_index_create builds the split-bf16 ref image
                          * and norms whatever the path bits say (the 1-NN path stays what they say), and
                          * nns_index_range_count / _fill flag, per query, the 32-ref blocks whose split-bf16 score lies
                          * within a per-query threshold, then evaluate V0's distance only there.  Same lims, indices and
                          * distance bits as without the flag.  fp32 points whose filter form is the split one, 8 <= k <=
                          * 256, or bf16 points, 32 <= k <= 256 (exact operands on v_mfma_f32_16x16x32_bf16 over the
                          * order-1 image: one product per score); with NNS_FILTER_F32, NNS_FILTER_BF16 or another k:
                          * NNS_ERR_UNSUPPORTED.  Also accepted by nns_search_f32_range / nns_search_bf16_range */
    NNS_TOPK_MFMA = 8192,  /* top-K through the MFMA flag pass (K6m): nns_index_create builds the split-bf16 ref image and norms
                          * whatever the path bits say (the 1-NN path stays what they say), and nns_index_search_topk bounds
                          * each query's kn-th distance from a sample of the refs, flags the 32-ref blocks that can hold a ref
                          * within the bound, and selects among those with V0's arithmetic.  Same keys as without the flag.
                          * fp32 points whose filter form is the split one, 8 <= k <= 256, or bf16 points, 32 <= k <= 256
                          * (the ref image is then the bf16 filter's); with NNS_FILTER_F32, NNS_FILTER_BF16 or another k:
                          * NNS_ERR_UNSUPPORTED.  Also accepted by nns_search_f32_topk / nns_search_bf16_topk */
    NNS_FILTER_I8PRE_OFF = 16384, /* MFMA filter, fp32 points in the 128-deep lazy layout (64 < k <= 128 on split-bf16
                          * operands, default schedule): do not keep the int8 pre-pass's operands; every search runs the
                          * lazy 16x16x32 kernel.  Without the flag such an index also holds an int8 image of the centred
                          * refs under one scale and one i32 seed per ref (128 + 4 bytes per ref more), and each long-stream
                          * search chooses ON THE DEVICE between the int8 pre-pass kernel (first pass on
                          * v_mfma_i32_16x16x64_i8, half the MFMA cycles; flagged tiles refined with the lazy kernel's own
                          * chain) and the lazy kernel: the pre-pass runs when the refs' scale is valid and at most m / 64
                          * queries have an int8 bound above 1.5 x the lazy bound.  Same keys either way.  No effect at
                          * other depths or schedules; NNS_ERR_INVALID with other point types or with the force flag */
    NNS_FILTER_I8PRE_FORCE = 32768, /* ... run the pre-pass whenever the scale is valid, whatever the count says (the bound
                          * holds for any data: answers stay exact, an ill-suited cloud only refines more tiles) */
    NNS_MULTI_FORCE_COLLECTIVE = 256 /* nns_search_*_multi, for tests: no single-GPU shortcut — even ONE shard runs the
                          * thread-per-GPU body, ncclCommInitAll and the grouped ncclAllReduce (core.cu:965-1057's
                          * shape), so that branch can be executed on a one-GPU box (a 1-rank all-reduce) */
};

/*
 * Packed (distance, index) key: (fp32 bits of the V0 distance << 32) | index.
 * Distances are >= +0, so unsigned (and, below 2^63, signed) integer order is
 * (distance, then index) lexicographic order: min over keys == V0's argmin
 * rule at every reduction level, including an RCCL ncclMin
 * all-reduce on int64/uint64.  NNS_KEY_NONE marks "no selectable distance"
 * (V0 leaves minSum = INFINITY, index = 0: core.cu:34-35).
 */
typedef uint64_t nns_key;
#define NNS_KEY_NONE 0x7F80000000000000ull

/* Most points one set (queries of a search, refs of an index or whole call) may hold: 2^31 - 2^20.  The reference's
 * sizes and indices are `int` (core.cu:24-26); this library keeps int32 indices and leaves 2^20 of headroom below
 * 2^31 for padded tile images and range ends.  Larger m or n: NNS_ERR_INVALID (shard the refs with index_base). */
#define NNS_MAX_POINTS 0x7FF00000

/* opaque handle: one device-resident, prepared shard of reference points */
typedef struct nns_index nns_index;

/* per-search statistics.  NNS_PROFILE adds the *_ms fields (HIP events on the caller's stream):
 * averages over the searches since the previous nns_index_stats call (the last 32 at most), so
 * a caller can run many refresh + search steps back to back and read them once. */
typedef struct nns_stats {
    int path;              /* NNS_PATH_EXACT or NNS_PATH_MFMA actually taken */
    int k_tile;            /* K of the MFMA tile (k padded up), 0 on the exact path */
    int splits;            /* ref-range splits of the filter grid */
    int ambiguous;         /* queries re-ranked by the exact scan (filter margin < tau) */
    int nonfinite;         /* 1 if NaN/INF/huge inputs forced the exact path */
    float prep_refs_ms;    /* K2 on refs (index create) */
    float prep_queries_ms; /* K2 on queries */
    float filter_ms;       /* K3 MFMA filter */
    float finalize_ms;     /* K5 merge + exact distance of winners */
    float rerank_ms;       /* exact scan of ambiguous queries */
    float exact_ms;        /* exact path kernels (K1) */
    float total_ms;        /* all device work of a search */
    int multi_candidate;   /* queries whose filter margin was below tau: K5 chose among > 1 candidates with
                            * V0's arithmetic (nns_index_near_ties lists them) */
} nns_stats;

/* ---- whole-call drop-ins (host pointers; alloc + H2D + kernels + D2H) ------ */

/* Replaces vN::cudaCall (core.cu:23-29): *results is malloc()'d (m ints) and
 * owned by the caller (free()).  Uses device 0.  Returns NNS_OK or an error
 * (never exits). */
int nns_search_f32(int k, int m, int n, const float *s_points,
                   const float *r_points, int **results);

/* Same search into caller-provided host buffers; dist_out may be NULL.
 * num_shards > 1 splits the refs into contiguous ceil(n/num_shards) ranges
 * (the V8/V9 split rule, core.cu:781-791) searched one after another on the
 * one device and merged with nns_keys_min — the single-GPU rehearsal of the
 * multi-GPU path.  flags: NNS_PATH_*. */
int nns_search_f32_ex(int k, int m, int n, const float *s_points,
                      const float *r_points, int *idx_out, float *dist_out,
                      int num_shards, unsigned flags, int device);

/* The V8/V9 analogue (core.cu:761-853, 965-1057): refs sharded contiguously over
 * num_devices GPUs (<= 0: all visible) by one host thread per GPU, per-GPU packed
 * keys combined with ONE RCCL min all-reduce (uint64, ncclMin) over xGMI; falls back
 * to one GPU for small problems exactly as the reference does (core.cu:775-777:
 * n <= min(2^18, 1024 m)).  Result = V0's, for every m (the reference's own merge
 * is wrong for m > 1).  The RCCL communicators of a device set are created
 * on the first call and cached for the life of the process (nns_shutdown() destroys
 * them); concurrent multi calls of one process are serialised around the collective.
 * NNS_REFS_SOA is accepted (a shard is then a column range of the [k][n] array).  m or n above
 * NNS_MAX_POINTS: NNS_ERR_INVALID, before anything is allocated.  The caller's current device is
 * restored on return. */
int nns_search_f32_multi(int k, int m, int n, const float *s_points,
                         const float *r_points, int *idx_out, float *dist_out,
                         int num_devices, unsigned flags);
int nns_search_bf16_multi(int k, int m, int n, const uint16_t *s_points,
                          const uint16_t *r_points, int *idx_out, float *dist_out,
                          int num_devices, unsigned flags);
/* Diagnostic: the number of ranks of the last grouped RCCL all-reduce an nns_search_*_multi call of this process
 * completed (0: none yet, or the keys were merged through the host instead). */
int nns_multi_last_exchange_ranks(void);

/* ---- split API (device-resident buffers, caller's stream) ------------------ */

/* Prepare a shard of n reference points r_dev[n][k] (device memory, fp32 AoS)
 * for searching.  index_base is added to every returned index (the shard's
 * offset into the global ref set, core.cu:827-829).  r_dev must stay valid and
 * unchanged for the life of the index (the exact re-rank reads the original
 * values).  stream: a hipStream_t (NULL = default stream). */
int nns_index_create(nns_index **out, int device, int k, int n,
                     const float *r_dev, int64_t index_base, unsigned flags,
                     void *stream);
int nns_index_destroy(nns_index *ix);

/* Re-run the reference pre-pass (K2) on the same buffer, e.g. after the caller
 * rewrote r_dev in place, or to time it. */
int nns_index_refresh(nns_index *ix, void *stream);

/* keys_dev[i] = packed (V0 distance, index_base + argmin) of query i over this
 * shard, or NNS_KEY_NONE.  q_dev[m][k] fp32 AoS in device memory. */
int nns_index_search(nns_index *ix, int m, const float *q_dev,
                     nns_key *keys_dev, void *stream);

/* bf16 points (config C5: bf16 inputs, fp32 accumulate).  Arrays hold raw bf16 bit
 * patterns (uint16_t), same [points][k] layout.  Semantics: V0's arithmetic on the
 * bf16 values widened to fp32 (the reference has no bf16 code; SURVEY 8c defines the
 * oracle this way).  MFMA filter for 32 <= k <= 1024 (v_mfma_f32_16x16x32_bf16 up to 256,
 * v_mfma_f32_32x32x16_bf16 beyond), exact kernels otherwise.  An index and its queries must have the same dtype. */
int nns_index_create_bf16(nns_index **out, int device, int k, int n,
                          const uint16_t *r_dev, int64_t index_base,
                          unsigned flags, void *stream);
int nns_index_search_bf16(nns_index *ix, int m, const uint16_t *q_dev,
                          nns_key *keys_dev, void *stream);
int nns_search_bf16_ex(int k, int m, int n, const uint16_t *s_points,
                       const uint16_t *r_points, int *idx_out, float *dist_out,
                       int num_shards, unsigned flags, int device);

/* fp16 points (IEEE binary16: stored embeddings, point clouds).  Arrays hold raw binary16 bit patterns (uint16_t),
 * same [points][k] layout.  Semantics: the bf16 contract with one word changed — V0's arithmetic on the values widened
 * exactly to fp32 (subnormals, INF and NaN included); indices bit-exact, distances bit-equal, lowest index wins ties,
 * NaN and +INF distances never selected.  An index and its queries must have the same dtype: an fp16 index searched
 * through nns_index_search / nns_index_search_bf16 (or an fp32 / bf16 index through nns_index_search_f16) returns
 * NNS_ERR_INVALID.  The dtype-agnostic entry points (nns_index_search_indices, nns_index_search_topk,
 * nns_index_range_count / nns_index_range_fill, nns_index_refresh, nns_index_stats, nns_index_near_ties) serve an fp16
 * index like any other; top-K, range search and the nns_keys_* helpers keep their contracts.
 * Flags: NNS_PATH_AUTO / NNS_PATH_EXACT / NNS_PATH_MFMA, NNS_PROFILE, NNS_REFS_SOA, NNS_RECORDS_PER_REF.  The operand
 * flags of fp32 points (NNS_FILTER_BF16, NNS_FILTER_F32, NNS_FILTER_SPLIT_EAGER): NNS_ERR_INVALID, as for bf16 points.
 * NNS_RANGE_MFMA and NNS_TOPK_MFMA are not built for fp16 points: NNS_ERR_UNSUPPORTED (at create, in the whole calls and
 * in nns_plan_filter), answered like the operand flags before the device is looked up.
 * MFMA filter: 32 <= k <= 256 with at least 64 queries (the AUTO rule of bf16 points), on v_mfma_f32_16x16x32_f16 at
 * KT = 128 / 256 over K2's order-1 image of binary16 operands; two binary16 values multiply exactly in fp32, so the margin
 * is the exact-operand one (nns_tau_consts mode 4, nns_index_filter_form 4).  k < 32 and 256 < k <= 16384 take the exact
 * kernels under AUTO; NNS_PATH_MFMA with k > 256: NNS_ERR_UNSUPPORTED.
 * Range guard: the ref image holds -2 v narrowed to binary16, finite only for |v| <= 32752.  Refs with a larger value
 * (32768 .. 65504), like NaN and INF, void the filter: the index searches with the exact kernels and
 * nns_stats.nonfinite reads 1.  Queries are not scaled: only their NaN / INF matter (those searches re-rank every query
 * with the exact scan, as for the other dtypes).
 * Measured on the MI355X (tests/test_f16_gpu.py; DESIGN section 4, "fp16 points"): the f16 MFMA's worst
 * |hardware - fp64| is 0.0143 (KT = 128) / 0.0102 (KT = 256) of the mode-4 e3 bound, against the 1/4 allowed, so the
 * allowance stays 2u per add.  Subnormal binary16 operands (|v| < 2^-14, nonzero) are NOT flushed by the f16 MFMA
 * (all-subnormal and every-tenth-subnormal operands: 0.0049 / 0.0037 of the bound): they go through the filter like
 * any value, with no void condition and no floor in tau.  Times (tools/probe_f16.py, profiles/f16_probe.json, next to a
 * bf16 index on the same values rounded to bf16): 4096 x 1 M x 128 0.845 ms per search (filter 0.758 ms) against 0.806
 * (0.718) ms, the f16 filter 5.6 % slower; 65536 x 65536 x 32 0.815 against 0.807 ms, equal within the rounds' spread. */
int nns_index_create_f16(nns_index **out, int device, int k, int n,
                         const uint16_t *r_dev, int64_t index_base,
                         unsigned flags, void *stream);
int nns_index_search_f16(nns_index *ix, int m, const uint16_t *q_dev,
                         nns_key *keys_dev, void *stream);
int nns_search_f16_ex(int k, int m, int n, const uint16_t *s_points,
                      const uint16_t *r_points, int *idx_out, float *dist_out,
                      int num_shards, unsigned flags, int device);

/* int8 points (quantised embeddings, 8-bit descriptors).  Arrays are const int8_t *, same [points][k] layout.
 * Semantics: the fp16 contract with one word changed — V0's arithmetic on the values widened exactly to fp32; indices
 * bit-exact, distances bit-equal, lowest index wins ties, index 0 when nothing is selectable.  An index and its queries
 * must have the same dtype: any mix with the fp32 / bf16 / fp16 entry points returns NNS_ERR_INVALID.  The dtype-agnostic
 * entry points (nns_index_search_indices, nns_index_search_topk, nns_index_range_count / nns_index_range_fill,
 * nns_index_refresh, nns_index_stats, nns_index_near_ties) serve an int8 index like any other.
 * Exactness: each |q - r| <= 255, so a squared term is at most 65 025 and any sum of at most 256 of them at most
 * 16 646 400 < 2^24: for k <= 256 V0's fp32 chain never rounds and the V0 distance IS the integer squared distance.
 * (Beyond k = 258 the chain does round; the contract covers that: the exact kernels run V0's own arithmetic.)
 * int8 has no non-finite or out-of-range value: nns_stats.nonfinite is always 0, and there is NO void or guard condition
 * for refs or queries.
 * Flags: NNS_PATH_AUTO / NNS_PATH_EXACT / NNS_PATH_MFMA, NNS_PROFILE, NNS_RECORDS_PER_REF.  NNS_FILTER_BF16,
 * NNS_FILTER_F32 and NNS_FILTER_SPLIT_EAGER: NNS_ERR_INVALID.  NNS_RANGE_MFMA, NNS_TOPK_MFMA and NNS_REFS_SOA are not
 * built for int8 points: NNS_ERR_UNSUPPORTED (at create, in the whole calls and in nns_plan_filter), answered like the
 * operand flags before the device is looked up.
 * MFMA filter: 32 <= k <= 256 with at least 64 queries (the AUTO rule of the 16-bit types), on v_mfma_i32_16x16x64_i8
 * with i32 accumulators at KT = 256 for every such k (k <= 128 pads to 256: no 128-deep form is built) over K2's int8
 * image — the values themselves, the factor -2 is applied where a tile retires.  The score |y|^2 - 2 x.y is an integer
 * of magnitude < 2^24, exact in the accumulator and exact as fp32: the hardware contributes no error to the margin.
 * nns_index_filter_form reports 5; the margin formula is nns_tau_consts mode 1's (there is no mode 5).  k < 32 and
 * 256 < k <= 16384 take the exact kernels under AUTO; NNS_PATH_MFMA with k > 256: NNS_ERR_UNSUPPORTED.
 * Times (tools/probe_i8.py, profiles/i8_probe.json): see README. */
int nns_index_create_i8(nns_index **out, int device, int k, int n,
                        const int8_t *r_dev, int64_t index_base,
                        unsigned flags, void *stream);
int nns_index_search_i8(nns_index *ix, int m, const int8_t *q_dev,
                        nns_key *keys_dev, void *stream);
int nns_search_i8_ex(int k, int m, int n, const int8_t *s_points,
                     const int8_t *r_points, int *idx_out, float *dist_out,
                     int num_shards, unsigned flags, int device);

/* uint8 points (SIFT / BIGANN descriptors, raw pixels, 8-bit quantisers: values 0 .. 255).  dtype code 5 (the bf16_points
 * argument of nns_plan_filter / nns_plan_topk / nns_plan_range).  Arrays are const uint8_t *, same [points][k] layout.
 * Semantics: the int8 contract with one word changed — V0's arithmetic on the values widened exactly to fp32; indices
 * bit-exact, distances bit-equal, lowest index wins ties, index 0 when nothing is selectable; nns_stats.nonfinite is
 * always 0 and there is NO void or guard condition.  For k <= 256 the distance is the exact integer squared distance, at
 * most 256 * 255^2 = 16 646 400 < 2^24; beyond k = 258 V0's chain rounds and the exact kernels run V0's own arithmetic
 * (k <= 16384).  An index and its queries must have the same dtype: any mix with the other dtypes' entry points returns
 * NNS_ERR_INVALID, in both directions.  The dtype-agnostic entry points serve a uint8 index like any other.
 * Bias identity: (q - 128) - (r - 128) = q - r for every coordinate, so every term of V0's chain on the widened uint8
 * values is the fp32 integer it is on the int8 values q - 128, r - 128.  K2 flips the top bit of each byte (u ^ 0x80 read
 * as int8 is u - 128) and so builds exactly the int8 operand image: for 32 <= k <= 256 and at least 64 queries the
 * filter is the int8 one, unchanged (v_mfma_i32_16x16x64_i8 at KT = 256, exact integer scores, |x'.y'| <= 2^22,
 * |score| < 2^24, the margin nns_tau_consts mode 1's); nns_index_filter_form reports 5.  The padded dimensions hold 0
 * after the bias in queries and refs alike; the norms are the sums of (u - 128)^2 over the real dimensions.
 * Flags: NNS_PATH_AUTO / NNS_PATH_EXACT / NNS_PATH_MFMA, NNS_PROFILE, NNS_RECORDS_PER_REF, NNS_RANGE_MFMA and
 * NNS_TOPK_MFMA (32 <= k <= 256: K7m / K6m on the int8 MFMA, below; other k: NNS_ERR_UNSUPPORTED).  NNS_FILTER_BF16,
 * NNS_FILTER_F32, NNS_FILTER_SPLIT_EAGER and the int8 pre-pass flags: NNS_ERR_INVALID.  NNS_REFS_SOA, and NNS_PATH_MFMA
 * with k > 256: NNS_ERR_UNSUPPORTED.  All of these are answered before the device is looked up.  There is no
 * nns_search_u8_multi.  Times (tools/probe_u8.py, profiles/u8_probe.json): see README. */
int nns_index_create_u8(nns_index **out, int device, int k, int n,
                        const uint8_t *r_dev, int64_t index_base,
                        unsigned flags, void *stream);
int nns_index_search_u8(nns_index *ix, int m, const uint8_t *q_dev,
                        nns_key *keys_dev, void *stream);
int nns_search_u8_ex(int k, int m, int n, const uint8_t *s_points,
                     const uint8_t *r_points, int *idx_out, float *dist_out,
                     int num_shards, unsigned flags, int device);

/* Binary points ("b1": ORB / BRIEF descriptors, 1-bit quantised embeddings) under Hamming distance.  dtype code 4 (the
 * bf16_points argument of nns_plan_topk / nns_plan_range).
 * Storage: a point of k bits is k / 32 consecutive uint32_t words, 4-byte aligned; bit t of a point is
 * (word[t / 32] >> (t % 32)) & 1 — on a little-endian host numpy.packbits(..., bitorder="little").  Layout
 * [points][k / 32], row-major.  k is the number of BITS in every entry point and plan call.
 * Limits: k % 32 != 0: NNS_ERR_UNSUPPORTED (pad both sets with zero bits: no distance changes).  k / 32 > 16384:
 * NNS_ERR_UNSUPPORTED (the exact path's own limit, applied to words).  A point set that is not 4-byte aligned:
 * NNS_ERR_INVALID.
 * Semantics: the int8 contract with one word changed — V0's arithmetic on the bits widened to 0.0 / 1.0.  Every term
 * fl(fl(q - r)^2) is then 0 or 1 and every partial sum an integer <= k <= 2^19 < 2^24, so V0's distance IS
 * popcount(q xor r), the Hamming distance, as fp32: indices bit-exact, distances bit-equal, lowest index wins ties, index
 * 0 when nothing is selectable.  nns_stats.nonfinite is always 0; there is NO void or guard condition.  An index and
 * its queries must have the same dtype: any mix with the fp32 / bf16 / fp16 / int8 entry points returns
 * NNS_ERR_INVALID, in both directions.  The dtype-agnostic entry points (nns_index_search_indices,
 * nns_index_search_topk, nns_index_range_count / nns_index_range_fill, nns_index_refresh, nns_index_stats,
 * nns_index_near_ties — count 0 —, nns_index_topk_info / nns_index_range_info) serve a b1 index like any other, q_dev
 * in the index's dtype.
 * Path: there is no MFMA filter: always NNS_PATH_EXACT, nns_index_filter_form reports -1.  The lane-per-ref scans
 * (K1b, K6, K7) run one xor and one accumulating popcount per 32-bit word.
 * Flags: NNS_PATH_AUTO / NNS_PATH_EXACT, NNS_PROFILE.  NNS_PATH_MFMA, NNS_RANGE_MFMA, NNS_TOPK_MFMA, NNS_REFS_SOA and
 * NNS_RECORDS_PER_REF: NNS_ERR_UNSUPPORTED.  NNS_FILTER_BF16, NNS_FILTER_F32 and NNS_FILTER_SPLIT_EAGER:
 * NNS_ERR_INVALID.  All of these, like the limits on k and the alignment, are answered before the device is looked up.
 * nns_search_*_multi is not extended to binary points.
 * Times (tools/probe_b1.py, profiles/b1_probe.json): see README. */
int nns_index_create_b1(nns_index **out, int device, int k, int n,
                        const uint32_t *r_dev, int64_t index_base,
                        unsigned flags, void *stream);
int nns_index_search_b1(nns_index *ix, int m, const uint32_t *q_dev,
                        nns_key *keys_dev, void *stream);
int nns_search_b1_ex(int k, int m, int n, const uint32_t *s_points,
                     const uint32_t *r_points, int *idx_out, float *dist_out,
                     int num_shards, unsigned flags, int device);

/* nns_index_search + nns_keys_unpack in one call for the single-shard case (what the reference's
 * cudaCall hands back is indices): keys_dev[m] as above AND idx_dev[m] = index of each key (0 for
 * NNS_KEY_NONE, as V0), dist_dev (optional) = its fp32 distance.  The low-dimensional exact kernel
 * writes all three in its one launch; the other paths append the unpack kernel.  q_dev has the
 * index's dtype (fp32, bf16 / fp16 bit patterns, int8, or packed bits). */
int nns_index_search_indices(nns_index *ix, int m, const void *q_dev, nns_key *keys_dev,
                             int *idx_dev, float *dist_dev, void *stream);

int nns_index_stats(nns_index *ix, nns_stats *out);

/* The queries of the LAST nns_index_search on the MFMA path whose answer was NOT settled by the
 * filter alone: more than one reference lay within the proof margin tau of the filter's minimum and
 * K5 decided among them with V0's exact arithmetic (queries sent to the exact scan are counted by
 * nns_stats.ambiguous instead).  *count_out = how many; up to `cap` query numbers are copied into
 * ids_out (host memory, any order).  Synchronises the device.  These are the queries a parity check
 * at sizes beyond the oracle's reach should verify in full (SURVEY 8d's "filter margin" gate). */
int nns_index_near_ties(nns_index *ix, int *ids_out, int cap, int *count_out);

/* inout[i] = min(inout[i], other[i]) : the cross-shard merge operator. */
int nns_keys_min(nns_key *inout_dev, const nns_key *other_dev, int m, void *stream);

/* idx_dev[i] = index of keys_dev[i] (0 for NNS_KEY_NONE, as V0); dist_dev
 * (optional) = its fp32 distance (+INF for NNS_KEY_NONE). */
int nns_keys_unpack(const nns_key *keys_dev, int m, int *idx_dev,
                    float *dist_dev, void *stream);

/* ---- k nearest neighbours (top-K) --------------------------------------------
 * Semantics: for query i, the kn references with the smallest V0 distance (the value nns_index_search computes:
 * sum_{t ascending} fl(fl(q - r)^2), un-contracted fp32 from 0), ordered by ascending (distance, global index) —
 * the first kn entries of a stable sort by V0 distance, which is plain key order.  A NaN or +INF distance is never
 * selected (V0's rule, in every slot).  When fewer than kn references are selectable (n < kn, non-finite data) the
 * row is padded with NNS_KEY_NONE, which nns_keys_topk_unpack turns into index -1 and distance +INF.  Distances are
 * bit-equal to V0's; indices are global (index_base added).  kn = 1 gives keys bit-identical to nns_index_search.
 * Supported: 1 <= kn <= NNS_TOPK_MAX (larger: NNS_ERR_UNSUPPORTED; kn <= 0: NNS_ERR_INVALID), fp32 and bf16 points,
 * every k the exact path accepts (k <= 16384).  The exact scan (K6) runs whatever path the index was created for;
 * its ref-split workspace (at most 256 MiB) belongs to the index and grows on demand. */
#define NNS_TOPK_MAX 256

/* keys_dev[m][kn] = the kn nearest refs of each query as packed keys, ascending.  q_dev has the index's dtype.
 * Reads the index's point-major refs.  nns_index_stats then reports NNS_PATH_EXACT (with NNS_PROFILE, exact_ms /
 * total_ms cover the scan and merge); an NNS_TOPK_MFMA index: see below.  Same one-index-per-stream rule as nns_index_search. */
int nns_index_search_topk(nns_index *ix, int m, const void *q_dev, int kn, nns_key *keys_dev, void *stream);
/* Per row i of [m][kn]: inout[i] = the kn smallest keys of the union of the ascending rows inout[i] and other[i]
 * (shards with disjoint index ranges): the top-K form of nns_keys_min. */
int nns_keys_topk_merge(nns_key *inout_dev, const nns_key *other_dev, int m, int kn, void *stream);
/* idx_dev[m][kn] = index of each key (-1 for NNS_KEY_NONE); dist_dev (optional) = its fp32 distance (+INF for
 * NNS_KEY_NONE). */
int nns_keys_topk_unpack(const nns_key *keys_dev, int m, int kn, int *idx_dev, float *dist_dev, void *stream);
/* Whole calls: host buffers, idx_out[m][kn], dist_out[m][kn] optional.  num_shards > 1: the V8/V9 contiguous split
 * searched one after another on the one device and merged with nns_keys_topk_merge (as nns_search_f32_ex).  flags:
 * NNS_PATH_AUTO, NNS_PATH_EXACT, NNS_REFS_SOA, NNS_PROFILE, and NNS_TOPK_MFMA (below: fp32 points at 8 <= k <= 256, bf16
 * points at 32 <= k <= 256); any other:
 * NNS_ERR_UNSUPPORTED.  Library stream, no
 * device-wide synchronisation, caller's device restored, NNS_MAX_POINTS checked before anything is allocated. */
int nns_search_f32_topk(int k, int m, int n, const float *s_points, const float *r_points, int kn, int *idx_out,
                        float *dist_out, int num_shards, unsigned flags, int device);
int nns_search_bf16_topk(int k, int m, int n, const uint16_t *s_points, const uint16_t *r_points, int kn,
                         int *idx_out, float *dist_out, int num_shards, unsigned flags, int device);
/* fp16 points (binary16 bit patterns): the same call; NNS_TOPK_MFMA: NNS_ERR_UNSUPPORTED. */
int nns_search_f16_topk(int k, int m, int n, const uint16_t *s_points, const uint16_t *r_points, int kn,
                        int *idx_out, float *dist_out, int num_shards, unsigned flags, int device);
/* int8 points: the same call; NNS_TOPK_MFMA: NNS_ERR_UNSUPPORTED. */
int nns_search_i8_topk(int k, int m, int n, const int8_t *s_points, const int8_t *r_points, int kn,
                       int *idx_out, float *dist_out, int num_shards, unsigned flags, int device);
/* uint8 points: the same call; NNS_TOPK_MFMA at 32 <= k <= 256 runs K6m on the int8 MFMA (other k: NNS_ERR_UNSUPPORTED). */
int nns_search_u8_topk(int k, int m, int n, const uint8_t *s_points, const uint8_t *r_points, int kn,
                       int *idx_out, float *dist_out, int num_shards, unsigned flags, int device);
/* binary points (k in bits, packed words): the same call; every flag but the auto / exact path and NNS_PROFILE:
 * see nns_index_create_b1. */
int nns_search_b1_topk(int k, int m, int n, const uint32_t *s_points, const uint32_t *r_points, int kn,
                       int *idx_out, float *dist_out, int num_shards, unsigned flags, int device);
/* Diagnostic (host only, no device needed): the top-K launch geometry for a k-D search of m queries over n refs.
 * out[0..5] = {queries per workgroup, ref splits (grid.y), refs per split, workgroups, LDS bytes per workgroup,
 * split-workspace keys (0 with one split)}.  bf16_points: 0 fp32, 1 bf16, 2 fp16, 3 int8, 5 uint8 points (the narrow types
 * share one geometry: their refs are widened as they are read), 4 binary points: k is in bits, and the LDS and workspace fields
 * follow k / 32 words of 4 bytes (k % 32 != 0 or k / 32 > 16384: NNS_ERR_UNSUPPORTED). */
int nns_plan_topk(int k, int m, int n, int kn, int bf16_points, int *out, int out_len);

/* ---- top-K on the matrix cores (NNS_TOPK_MFMA, K6m) -------------------------------
 * On an index created with NNS_TOPK_MFMA, nns_index_search_topk keeps every contract above (ascending (distance, index)
 * keys, bit-equal V0 distances, NaN / +INF never selected, NNS_KEY_NONE padding, index_base) and runs in three steps.
 * Bound: K6's scan over every stride-th 32-ref block gives U_i, the kn-th smallest V0 distance of that sample; the kn-th
 * smallest over all refs cannot be larger.  Flag: K7m's flag pass with radius2 = U_i per query sets the bit of every
 * block that can hold a ref with d <= U_i (nns_range_threshold).  Select: V0's distance for the refs of flagged blocks
 * only, on the original points, the kn smallest keys kept.  The flag bitmap is the one NNS_RANGE_MFMA uses (at most
 * 256 MiB, query batches beyond), the per-chunk lists use the top-K split workspace; keys_dev holds the sample's rows
 * in between.  K6 runs instead, decided on the host, when m < 64, the refs hold NaN / INF / |v| >= 1e17, the sample
 * rule leaves a stride below 2 (few refs for the kn asked), or the flag pass has no plan for the shape.  A QUERY whose
 * bound is not finite or whose values void the filter's error model gets its flag row filled: its selection is the
 * exact scan.  nns_index_stats reports NNS_PATH_MFMA after a filtered search; with NNS_PROFILE rerank_ms holds the
 * bound scan (K6 on the sample), prep_queries_ms K2 on the queries, filter_ms the flag pass, finalize_ms the selection
 * and merge (several batches: filter_ms covers all but the last batch's selection).
 * bf16 points (32 <= k <= 256): the same three steps; the bound scan and the selection widen the bf16 values as K6
 * does, the flag pass is K7m's for bf16 points (below). */

/* Diagnostic: what the last nns_index_search_topk on this index did.  out[0..3] = {path taken (NNS_PATH_EXACT: K6,
 * NNS_PATH_MFMA: K6m), flagged (query, 32-ref block) pairs, pairs examined (m x blocks per query), queries whose flag
 * row was filled}; the last three are 0 on the exact path, all four before any top-K search.  out_len >= 4.  Waits for
 * the stream the index last worked on (not the device). */
int nns_index_topk_info(nns_index *ix, int64_t *out, int out_len);
/* Diagnostic (host only, no device needed): the plan of K6m for a k-D search of m queries over n refs at kn, index flags
 * `flags`.  out[0..16] = {sample blocks, block stride (0: fewer blocks than the rule asks for), sample refs, filtered
 * (1: K6m; 0: K6 — stride < 2, m < 64, or no flag-pass plan), then with filtered = 1 (else zeros) the ten fields of
 * nns_plan_range_mfma, selection chunks per query, flag words per chunk}, and out[16] = LDS bytes of a selection
 * workgroup.  The sample: sb = max(ceil(sqrt(kn n max(k, 16) / 512)), ceil(max(2048, 16 kn) / 32)) blocks asked for (a
 * selected ref weighs max(k, 16) / 16 scanned ones; at most every second block unless the unweighted rule asks for more),
 * stride = floor(ceil(n / 32) / sb), the blocks b with b % stride == 0 taken.  out_len >= 17.  NNS_ERR_UNSUPPORTED for k outside
 * 8 .. 256, kn above NNS_TOPK_MAX, NNS_FILTER_F32, NNS_FILTER_BF16. */
int nns_plan_topk_mfma(int k, int m, int n, int kn, unsigned flags, int *out, int out_len);
/* The same plan for bf16 points: the same seventeen fields, the range fields those of nns_plan_range_mfma_bf16.
 * NNS_ERR_UNSUPPORTED for k outside 32 .. 256 or kn above NNS_TOPK_MAX; NNS_ERR_INVALID for the flags of fp32 points
 * (NNS_FILTER_F32, NNS_FILTER_BF16, NNS_FILTER_SPLIT_EAGER). */
int nns_plan_topk_mfma_bf16(int k, int m, int n, int kn, unsigned flags, int *out, int out_len);
/* K6m's plan for uint8 points: the same seventeen fields; kt is 256 and the layout field reads 3 (the int8 image). */
int nns_plan_topk_mfma_u8(int k, int m, int n, int kn, unsigned flags, int *out, int out_len);

/* ---- fixed-radius neighbours (range search) -----------------------------------
 * Semantics: a hit of query i is every reference j (global index, index_base added) whose V0 distance d (the value
 * nns_index_search computes: sum_{t ascending} fl(fl(q - r)^2), un-contracted fp32 from 0) satisfies d <= radius2,
 * compared in fp32, inclusive.  radius2 is the SQUARED radius, fp32 for both point types.  A NaN or +INF distance is
 * never a hit, even with radius2 = +INF.  radius2 NaN or < 0: NNS_ERR_INVALID; -0.0 counts as 0 (then only exact
 * duplicates of the query are hits).
 * Output, CSR in the lims form of FAISS's range search: int64 lims[m + 1] with lims[0] = 0 and lims[i + 1] - lims[i]
 * = the hit count of query i (at most n); query i's hits are idx[lims[i] .. lims[i + 1]) in ascending global index,
 * and the optional dist[...] holds their V0 distances, bit-equal to V0's.  Every position comes from counts, never
 * from the arrival order of atomics: two runs give identical buffers.  The total lims[m] may exceed 2^31.
 * Supported: what top-K supports — every k the exact path accepts (k <= 16384; larger: NNS_ERR_UNSUPPORTED), fp32 and
 * bf16 points, an index created for any path or with NNS_REFS_SOA (the range passes read its point-major refs).  The
 * exact scan (K7) runs two passes, count and fill.  Their workspace (per-(query, ref chunk) offsets and the scan of the
 * counts over m, at most 256 MiB) belongs to the index, grows on demand and is freed behind an event like the top-K
 * workspace.  Same one-index-per-stream rule as nns_index_search; nns_index_stats then reports NNS_PATH_EXACT (with
 * NNS_PROFILE, exact_ms / total_ms cover the pass). */

/* Count pass.  lims_dev[m + 1] (device, int64) receives the lims above.  The per-chunk counts the fill needs stay in
 * the index's range workspace.  q_dev has the index's dtype. */
int nns_index_range_count(nns_index *ix, int m, const void *q_dev, float radius2, int64_t *lims_dev, void *stream);
/* Fill pass.  Must follow nns_index_range_count on the same index with the same m, q_dev and radius2, and no other
 * range count in between; otherwise NNS_ERR_INVALID.  1-NN and top-K searches in between are allowed.  lims_dev: the
 * count's output (unchanged); idx_dev[lims[m]] (int32, device); dist_dev[lims[m]] optional.  A null idx_dev or
 * dist_dev is not written, so a fill after a count with lims[m] == 0 succeeds with the null pointer a zero-size
 * allocation returns (both null: nothing runs). */
int nns_index_range_fill(nns_index *ix, int m, const void *q_dev, float radius2, const int64_t *lims_dev,
                         int *idx_dev, float *dist_dev, void *stream);
/* Whole calls: count, read lims[m], allocate, fill.  lims_out: the caller's host int64[m + 1].  *idx_out (and
 * *dist_out when dist_out != NULL) are malloc()'d by the library with lims[m] entries, never NULL on success; the
 * caller free()s them.  On error both are set to NULL and nothing leaks; output beyond device or host memory gives
 * NNS_ERR_NOMEM.  flags: NNS_PATH_AUTO, NNS_PATH_EXACT, NNS_REFS_SOA, NNS_PROFILE, and NNS_RANGE_MFMA (below: fp32
 * points at 8 <= k <= 256, bf16 points at 32 <= k <= 256); any other: NNS_ERR_UNSUPPORTED.
 * Library stream, no device-wide synchronisation, caller's device restored, NNS_MAX_POINTS checked before anything is
 * allocated. */
int nns_search_f32_range(int k, int m, int n, const float *s_points, const float *r_points, float radius2,
                         int64_t *lims_out, int **idx_out, float **dist_out, unsigned flags, int device);
int nns_search_bf16_range(int k, int m, int n, const uint16_t *s_points, const uint16_t *r_points, float radius2,
                          int64_t *lims_out, int **idx_out, float **dist_out, unsigned flags, int device);
/* fp16 points (binary16 bit patterns): the same call; NNS_RANGE_MFMA: NNS_ERR_UNSUPPORTED. */
int nns_search_f16_range(int k, int m, int n, const uint16_t *s_points, const uint16_t *r_points, float radius2,
                         int64_t *lims_out, int **idx_out, float **dist_out, unsigned flags, int device);
/* int8 points: the same call; NNS_RANGE_MFMA: NNS_ERR_UNSUPPORTED. */
int nns_search_i8_range(int k, int m, int n, const int8_t *s_points, const int8_t *r_points, float radius2,
                        int64_t *lims_out, int **idx_out, float **dist_out, unsigned flags, int device);
/* uint8 points: the same call; NNS_RANGE_MFMA at 32 <= k <= 256 runs K7m on the int8 MFMA (other k: NNS_ERR_UNSUPPORTED). */
int nns_search_u8_range(int k, int m, int n, const uint8_t *s_points, const uint8_t *r_points, float radius2,
                        int64_t *lims_out, int **idx_out, float **dist_out, unsigned flags, int device);
/* binary points (k in bits, packed words; radius2 is compared with the Hamming distance as fp32): the same call. */
int nns_search_b1_range(int k, int m, int n, const uint32_t *s_points, const uint32_t *r_points, float radius2,
                        int64_t *lims_out, int **idx_out, float **dist_out, unsigned flags, int device);
/* Diagnostic (host only, no device needed): the range search's launch geometry for a k-D search of m queries over n
 * refs.  out[0..5] = {queries per workgroup, ref chunks (grid.y), refs per chunk, workgroups, LDS bytes per
 * workgroup, workspace bytes}.  bf16_points: 0 fp32, 1 bf16, 2 fp16, 3 int8, 5 uint8 points, 4 binary points (k in
 * bits; the fields follow k / 32 words, as in nns_plan_topk). */
int nns_plan_range(int k, int m, int n, int bf16_points, int *out, int out_len);

/* ---- range search on the matrix cores (NNS_RANGE_MFMA, K7m) ------------------------
 * On an index created with NNS_RANGE_MFMA the two range passes keep every contract above (lims form, ascending global
 * indices, bit-equal V0 distances, inclusive compare, NaN / +INF never a hit, fill matches the last count, searches in
 * between allowed, no atomically ordered positions, null idx_dev / dist_dev) and run in two steps: a flag pass on
 * v_mfma_f32_32x32x16_bf16 sets, per query, the bit of every 32-ref block that holds a split-bf16 score within the
 * query's threshold (nns_range_threshold); the evaluation pass computes V0's distance for the refs of flagged blocks
 * only, on the original points, and alone decides the hits.  The flag bitmap (m_pad x n_pad / 32 bits, at most
 * 256 MiB; beyond that the queries run in batches, the output order unchanged) belongs to the index, grows on demand
 * and is freed behind an event.  The passes fall back to K7, decided on the host, when m is below the filter's query
 * floor (64), the refs hold NaN / INF / |v| >= 1e17, or radius2 is not finite.  A QUERY with such values is known only
 * on the device: its flag row is filled, so the evaluation is the exact scan for it.  The whole call
 * nns_search_f32_range accepts the flag too (with NNS_PATH_AUTO / NNS_PATH_EXACT, NNS_REFS_SOA, NNS_PROFILE).
 * nns_index_stats reports NNS_PATH_MFMA after a filtered pass; with NNS_PROFILE prep_queries_ms is K2 on the queries,
 * filter_ms the flag pass, finalize_ms the evaluation (with several batches: filter_ms covers all but the last
 * batch's evaluation).
 * bf16 points (32 <= k <= 256, the depths of the 16x16x32 tiles; nns_search_bf16_range takes the flag too): the flag
 * pass runs v_mfma_f32_16x16x32_bf16 on K2's order-1 image, the one the 1-NN bf16 filter reads.  The operands are the
 * points themselves, so a score is ONE product per k-step — no hi / lo parts, no centring — and the threshold is
 * nns_range_threshold_bf16's.  Ring, bitmap, batches, evaluation, fallbacks, info and stats are the same.
 * uint8 points (32 <= k <= 256; nns_search_u8_range / nns_search_u8_topk take the flags too): the flag pass
 * (range_flag_u8_kernel) runs v_mfma_i32_16x16x64_i8 at depth 256 on K2's int8 image of the values biased by 128, the one
 * the 1-NN filter of a uint8 index reads.  Score and distance are exact integers, so the threshold is exact
 * (nns_range_threshold_u8) and a block is flagged if and only if it holds a hit.  No value voids the filter: the
 * fall-backs are m < 64, radius2 = +INF and, for K6m, a sample stride below 2.  The rest is the same. */

/* Diagnostic: what the last nns_index_range_count on this index did.  out[0..3] = {path taken (NNS_PATH_EXACT: K7,
 * NNS_PATH_MFMA: K7m), flagged (query, 32-ref block) pairs, pairs examined (m x blocks per query), total hits
 * lims[m]}; the middle two are 0 on the exact path, all four before any count.  out_len >= 4.  Waits for the stream
 * the index last worked on (not the device), like nns_index_near_ties. */
int nns_index_range_info(nns_index *ix, int64_t *out, int out_len);
/* Diagnostic (host only, no device needed): the launch geometry of K7m for a k-D search of m queries over n refs with
 * index flags `flags` (NNS_FILTER_SPLIT_EAGER selects the eager image layout).  out[0..9] = {tile depth kt, refs per
 * flagged block (32), blocks per query (n padded to K2's ring slot), queries per batch, batches, flag-workspace bytes,
 * grid.x of a full batch's flag pass, grid.y (ref-range splits), LDS bytes per workgroup, ref image layout (0 eager: hi,
 * lo fragments interleaved; 1 lazy: hi region, lo region)}.  out_len >= 10.  NNS_ERR_UNSUPPORTED outside the supported
 * forms (k outside 8 .. 256, NNS_FILTER_F32, NNS_FILTER_BF16, an n whose flag rows pass the workspace cap). */
int nns_plan_range_mfma(int k, int m, int n, unsigned flags, int *out, int out_len);
/* Diagnostic (host only): the score threshold K7m's flag pass gives a query of centred squared norm qnorm2 against
 * refs of maximum centred squared norm ymax2 at tile depth kt and squared radius radius2: with a = fl(radius2 - qnorm2),
 * fl(a + 1.002 tau(a)) (tau: nns_tau_consts mode 3) plus 2^-22 (radius2 + qnorm2).  Every ref with a V0 distance
 * <= radius2 has a score <= *thr_out.  Monotone in radius2. */
int nns_range_threshold(int kt, float qnorm2, float ymax2, float radius2, float *thr_out);
/* K7m's geometry for bf16 points: the same ten fields; kt is 128 or 256, and the layout field reads 2: the order-1
 * 16x16x32 image.  NNS_ERR_UNSUPPORTED for k outside 32 .. 256 (or an n whose flag rows pass the workspace cap);
 * NNS_ERR_INVALID for the flags of fp32 points (NNS_FILTER_F32, NNS_FILTER_BF16, NNS_FILTER_SPLIT_EAGER), as
 * nns_plan_filter answers them for bf16 points. */
int nns_plan_range_mfma_bf16(int k, int m, int n, unsigned flags, int *out, int out_len);
/* The threshold of a bf16 query (host only): the same form over nns_tau_consts mode 1 (exact operands), with qnorm2 the
 * query's own squared norm |x|^2 (no centring) and ymax2 the refs' largest |y|^2.  Every ref with a V0 distance
 * <= radius2 has a 16x16x32 score |y|^2 - 2 x.y <= *thr_out.  Monotone in radius2. */
int nns_range_threshold_bf16(int kt, float qnorm2, float ymax2, float radius2, float *thr_out);
/* K7m's geometry for uint8 points: the same ten fields, planned through nns_plan_filter's int8 geometry: kt is 256 for
 * every k, the block bytes (and every other field) are the bf16 plan's at depth 128, and the layout field reads 3: the
 * int8 image.  Rejections as nns_plan_range_mfma_bf16's. */
int nns_plan_range_mfma_u8(int k, int m, int n, unsigned flags, int *out, int out_len);
/* The threshold of a uint8 query (host only): thr = fl(floorf(fminf(radius2, 2^24)) - qnorm2), with qnorm2 the biased
 * squared norm |x - 128|^2 (an integer <= 2^22) that K2 keeps.  The score s = |y'|^2 - 2 x'.y' and the distance
 * d = qnorm2 + s are exact integers below 2^24 in magnitude and the subtraction is exact, so s <= thr <=> d <= radius2:
 * no margin.  radius2 >= 0, not NaN. */
int nns_range_threshold_u8(float qnorm2, float radius2, float *thr_out);

/* Deterministic synthetic clouds: dev[i] = u24(splitmix64(seed, offset+i)) * 2^-24
 * in [0,1) — bit-identical to oracle/v0_oracle.c:nns_rng_fill on the CPU. */
int nns_fill_uniform(float *dev, size_t count, uint64_t seed, uint64_t offset,
                     void *stream);

/* Diagnostic: one 32x32 tile through the filter's MFMA k-order.  a[32][kt],
 * b[32][kt], c0[32], out[32][32] are HOST fp32 buffers; out[i][j] = the MFMA
 * accumulation of sum_t a[i][t] * b[j][t] seeded with c0[i].  bf16 = 0:
 * v_mfma_f32_32x32x2_f32 (compared by the tests with a host fmaf() chain);
 * bf16 = 1: v_mfma_f32_32x32x16_bf16, bf16 = 2: four 16x16 tiles of v_mfma_f32_16x16x32_bf16
 * (the bf16 filter's shape and lane mapping), on the values cast to bf16 (compared with
 * fp64); bf16 = 3: the split chain of fp32 values (hi = rn_bf16(v), lo = rn_bf16(v - hi);
 * hi.hi + hi.lo + lo.hi per 16-dim step on v_mfma_f32_32x32x16_bf16, the default filter
 * form of fp32 points); bf16 = 5: four 16x16 tiles of v_mfma_f32_16x16x32_f16 in mode 2's lane mapping, on the values
 * cast to binary16 (the fp16 filter's shape; compared with fp64.  4 is taken: the lazy order behind
 * nns_selftest_mfma_lazy); bf16 = 6: four 16x16 tiles of v_mfma_i32_16x16x64_i8 in mode 2's lane mapping (the int8
 * filter's shape: kt a multiple of 64, operands cast to int8, the i32 accumulator seeded with (int)c0 and returned as
 * fp32 — exact integers: the check of the operand lane map).  These are the error models behind the filter's proof
 * margin tau. */
int nns_selftest_mfma(int kt, int bf16, const float *a, const float *b, const float *c0,
                      float *out);
/* The same tile in the order of the lazy split filter: the kt / 16 hi.hi MFMAs first — out_hh (optional) = the
 * accumulator at that point — then hi.lo and lo.hi of every 16-dim step on the same accumulator: out. */
int nns_selftest_mfma_lazy(int kt, const float *a, const float *b, const float *c0, float *out, float *out_hh);
/* The lazy split filter's chain on v_mfma_f32_16x16x32_bf16 (KT = 128): one wave, 32 refs x 64 queries.  q[64][128],
 * r[32][128], c0[32] are HOST fp32 buffers; the operands are taken from split images written in the 32x32x16 operand
 * order (as K2 writes them) through the kernel's own gather.  out_hh[ref][query] = the accumulator, seeded with c0[ref],
 * after the four hi.hi MFMAs; out[ref][query] = after rh.ql and rl.qh of every 32-dim step on top.  [32][64] each. */
int nns_selftest_mfma_lazy16(const float *q, const float *r, const float *c0, float *out, float *out_hh);
/* Diagnostic: the int8 pre-pass's operands and chain on one wave (host pointers; q [64][128], r [32][128] int8, seeds
 * [32]): the images are written in K2's lane map at depth 128, the refs negated, and the kernel's two
 * v_mfma_i32_16x16x64_i8 per tile run with the seeds as srcC.  out [32 refs][64 queries] = seeds[ref] - q.r, exact. */
int nns_selftest_mfma_i8pre(const int8_t *q, const int8_t *r, const int *seeds, int *out);
/* Diagnostic (host only): the MFMA tile of the lazy split kernel this build launches — 16 (v_mfma_f32_16x16x32_bf16, the
 * default) or 32 (v_mfma_f32_32x32x16_bf16, a build with -DNNS_F_LAZY_T16=0).  Plans, images and lists are the same. */
int nns_filter_lazy_tile(void);
/* Diagnostic (host only, no device needed): the launch geometry the MFMA filter would use for a k-D search of
 * m queries over n refs.  out[0..11] = {tile depth kt, bf16 operands, fp32 points rounded to bf16 operands,
 * candidate lists per query, m_pad, n_pad, ring slots in total, ref-range splits (grid.y), slots per split,
 * query groups (grid.x), refs per ring slot, queries per workgroup}; with out_len >= 14 also {lanes of a query
 * share thresholds, records per ref tile} (the short-stream forms); with out_len >= 15 also {fp32 points through
 * split-bf16 operands} (the geometry fields are the same for both fp32-point forms); with out_len >= 16 also {the split
 * operands run the lazy schedule} (0 with NNS_FILTER_SPLIT_EAGER, at depths without the lazy kernel and on the
 * short-stream record forms; the other fields do not depend on it).  NNS_ERR_UNSUPPORTED beyond
 * the deepest tile; NNS_ERR_INVALID for NNS_FILTER_BF16 / NNS_FILTER_F32 / NNS_FILTER_SPLIT_EAGER with bf16 points or together.  Lets CPU tests check the planner's invariants (coverage, padding, whole blocks per split).
 * bf16_points: 0 fp32, 1 bf16, 2 fp16 points.  fp16 points plan as bf16 points do, field for field, at 32 <= k <= 256;
 * k > 256, NNS_RANGE_MFMA or NNS_TOPK_MFMA: NNS_ERR_UNSUPPORTED; the operand flags: NNS_ERR_INVALID.
 * 3 int8 points: kt = 256 for every k <= 256, every other field the bf16 plan's at a 128-deep tile (k <= 128) — the
 * int8 block has that tile's bytes and fragments; rejections as for fp16 points, NNS_REFS_SOA with them.
 * 4 binary points: NNS_ERR_UNSUPPORTED (no filter is built for them).
 * 5 uint8 points: int8's plan field for field; NNS_RANGE_MFMA / NNS_TOPK_MFMA are accepted at 32 <= k <= 256. */
int nns_plan_filter(int k, int m, int n, int bf16_points, unsigned flags, int *out, int out_len);
/* Diagnostic (host only, no device needed): the launch geometry of the EXACT path (the reference's V1-V7 kernels,
 * core.cu:58-696) for a k-D search of m queries over n refs.  out[0..5] = {kernel: 0 K1a (lane = query, exact), 1 K1f
 * (k <= 3 from 2^27 pairs: vector-ALU filter + V0 re-rank in the same launch), 2 K1b (lane = ref), 3 K1c (<= 4 queries:
 * the HBM-streaming form); query tiles (grid.x); ref ranges (grid.y, 0 = chosen at launch); refs per range; waves per
 * workgroup; queries per workgroup}.  refs_aligned: the refs are 16-byte aligned; have_workspace: the merge workspace
 * exists (without it K1a / K1f run one ref range per query tile).  Lets CPU tests check the planner's invariants. */
int nns_plan_exact(int k, int m, int n, int refs_aligned, int have_workspace, int *out, int out_len);
/* Diagnostic: what the filter's slow path does when the lanes that carry one query share their record
 * thresholds (short ref streams): out64[l] = min of in64 over the lanes l ^ 32 (tile16 = 0: 32x32 MFMA tiles)
 * or l ^ 16, l ^ 32, l ^ 48 (tile16 = 1: 16x16 tiles) — through the very row-swap instructions the kernel
 * uses.  HOST buffers of 64 floats.  A wrong lane pairing would hand a query another query's threshold. */
int nns_selftest_lane_share(int tile16, const float *in64, float *out64);
/* Diagnostic (host only): the constants of the proof margin tau(a) = c0 + c1 * max(a + x2, 0) the
 * filter and K5 use for a query of squared norm qnorm2 against refs of maximum squared norm ymax2 at
 * tile depth kt; mode 0 fp32 operands, 1 bf16 points, 2 fp32 points rounded to bf16 operands, 3 fp32 points
 * as split-bf16 operands, 4 fp16 points, exact operands on f16 tiles (mode 1's formula: binary16 products are exact in
 * fp32).
 * out3 = {c0, c1, x2}.  Lets the tests hold the measured MFMA error against the model. */
int nns_tau_consts(int kt, float qnorm2, float ymax2, int mode, float *out3);
/* Diagnostic (host only): B of the lazy split filter — the bound on how far a pair's three-product score can lie below
 * its hi.hi partial score (cross products + their accumulation + the rounding of thr + B), for a query of squared norm
 * qnorm2 against refs of maximum squared norm ymax2 at tile depth kt.  out1 = B. */
int nns_split_lazy_bound(int kt, float qnorm2, float ymax2, float *out1);
/* The operand form of the index's MFMA filter, as its tau mode: 0 fp32 operands (NNS_FILTER_F32, or a depth without
 * the split form), 1 bf16 points, 2 fp32 points rounded to bf16 operands, 3 fp32 points as split-bf16 operands, 4 fp16
 * points, 5 int8 points (exact integer scores on v_mfma_i32_16x16x64_i8; 5 is not a tau mode: the margin formula is
 * nns_tau_consts mode 1's); -1 on the exact path.  Host only. */
int nns_index_filter_form(nns_index *ix, int *form_out);
/* *ran_out = 1 when the filter of the index's last search was the int8 pre-pass kernel (0: the lazy kernel, another
 * schedule or path, or no search yet).  A stream-ordered read: waits for the stream the index last worked on. */
int nns_index_filter_pre(nns_index *ix, int *ran_out);
/* B8 of the int8 pre-pass for one query: s the shared scale, ex2 = |e_x|^2 and q82 = |q8|^2 the
 * query's quantisation sums, r8max2 / eymax2 the refs' maxima, c0 = nns_tau_consts(128, ., ., 3)[0].  Host arithmetic. */
int nns_i8pre_bound(float s, float ex2, float q82, float r8max2, float eymax2, float c0, float *out1);

/* ---- the exchange of the one-process-per-GPU form ----------------------------
 * What V8/V9's gather + host re-rank (core.cu:821-852, 1025-1056) becomes when every GPU
 * has its own process (bench.py --gpus N under torch.distributed.run): each rank searches
 * its contiguous ref shard (nns_index_create with index_base = shard offset, core.cu:781-791,
 * :827-829) and the ranks combine their packed keys with ONE
 * ncclAllReduce(ncclUint64, ncclMin) over xGMI.  Same call site as nns_search_*_multi.
 *   rank 0:     nns_comm_unique_id(id, sizeof id)      (RCCL's ncclUniqueId, 128 bytes)
 *   caller:     carries the id bytes to every rank (MPI, a file, torch.distributed, ...)
 *   every rank: nns_comm_create(&c, id, sizeof id, nranks, rank, device)   (collective)
 *               nns_comm_allreduce_min(c, keys_dev, m, stream)            (async, in place)
 *               nns_comm_destroy(c)
 * librccl is dlopen()ed on first use; NNS_ERR_UNSUPPORTED if it cannot be loaded. */
#define NNS_COMM_ID_BYTES 128
typedef struct nns_comm nns_comm;
int nns_comm_unique_id(void *id_out, size_t id_bytes);
int nns_comm_create(nns_comm **out, const void *id, size_t id_bytes, int nranks,
                    int rank, int device);
int nns_comm_size(nns_comm *c);   /* ranks RCCL reports for the communicator (0 on error) */
int nns_comm_allreduce_min(nns_comm *c, nns_key *keys_dev, int m, void *stream);
int nns_comm_destroy(nns_comm *c);

/* ---- misc ------------------------------------------------------------------ */
int nns_device_count(void);
const char *nns_strerror(int status);
const char *nns_last_error(void); /* thread-local detail of the last failure */
int nns_version(void);            /* major * 1000 + minor */
/* Explicit replacement for the reference's hidden WarmUP static (ten V9 calls before main(),
 * core.cu:1900-1933): runs one tiny search through every kernel family (exact lane-per-query and
 * lane-per-ref, every fp32, bf16 and fp16 tile depth of the MFMA filter, the int8 tile and the Hamming scan of binary
 * points) on `device`, so that
 * code-object loading, the filter's LDS opt-in and the first pool allocations are paid here and
 * not inside a timed call.  Optional: every entry point works without it. */
int nns_warmup(int device);
/* The library parks freed device workspaces (queries/refs staging, tile images, candidate
 * lists) in a per-device pool instead of returning them to the runtime on every call — the
 * reference allocates and frees on every cudaCall (core.cu:793-802).  nns_trim() gives all
 * parked blocks back and returns the number of bytes released.  NNS_POOL_BYTES in the
 * environment caps what the pool may hold (default 16 GiB; 0 disables pooling). */
size_t nns_trim(void);
/* Destroys the cached RCCL communicators of nns_search_*_multi and trims the pool: call once
 * when the process is done with the library (optional; indexes and nns_comm handles are the
 * caller's to destroy). */
int nns_shutdown(void);

#ifdef __cplusplus
}
#endif
#endif /* NNS_MI355X_H */
