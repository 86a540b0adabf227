// nns_internal.h — shared declarations of the gfx950 nearest-neighbour kernels.
// (internal; the public boundary is include/nns.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <math.h>
#include <type_traits>
#include "nns.h"

namespace nns {

// ---- error plumbing ---------------------------------------------------------
void set_error(const char *fmt, ...);

#define NNS_HIP(call)                                                          \
    do {                                                                       \
        hipError_t nns_e_ = (call);                                            \
        if (nns_e_ != hipSuccess) {                                            \
            ::nns::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #call,     \
                             hipGetErrorString(nns_e_));                       \
            return NNS_ERR_HIP;                                                \
        }                                                                      \
    } while (0)

#define NNS_TRY(call)                                                          \
    do {                                                                       \
        int nns_s_ = (call);                                                   \
        if (nns_s_ != NNS_OK) return nns_s_;                                   \
    } while (0)

// ---- pooled device workspaces (dev_pool.hip) -----------------------------------
hipError_t pool_alloc(void **out, size_t bytes);
template <class T> static inline hipError_t pool_alloc(T **out, size_t bytes) { return pool_alloc((void **)out, bytes); }
void pool_free(void *ptr);     // caller has synchronised the work that used ptr
// ptr may still be in use by work already enqueued on `st`: reusable once an event recorded there has fired (no host wait)
void pool_free_after(void *ptr, hipStream_t st);
void pool_free_after(void *const *ptrs, int count, hipStream_t st);   // one event for all of them; nulls skipped
size_t pool_trim();            // give every parked block back to the runtime
// the library's own non-blocking streams (whole-call entry points); nullptr if none can be created
hipStream_t lib_stream_acquire();
void lib_stream_release(hipStream_t s);

// Every C-ABI entry point that selects a device restores the caller's current device on return (the reference's
// V8/V9 leave whatever cudaSetDevice they called last, core.cu:996; a library must not).
struct DeviceScope {
    int saved = -1;
    DeviceScope()
    {
        if (hipGetDevice(&saved) != hipSuccess) {
            (void)hipGetLastError();
            saved = -1;
        }
    }
    ~DeviceScope()
    {
        int cur = -1;
        if (saved >= 0 && hipGetDevice(&cur) == hipSuccess && cur != saved) (void)hipSetDevice(saved);
    }
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
};

// "the H2D copy that just returned (synchronous, legacy default stream) happens before whatever is enqueued on
// `st` next": an explicit event edge.  This runtime's pageable hipMemcpy returns after the device-side DMA, so the
// edge is already true here; CUDA documents the opposite for pageable sources and nothing in HIP's API promises it.
int order_after_default_stream(hipStream_t st);
void stager_release();         // free the small whole calls' pinned scratch (nns_api.hip)
// the overlapped upload of a contiguous host ref range (nns_api.hip), shared with nns_search_*_multi's shards
bool upload_overlap_pays(int k, int64_t m, int64_t n, int dtype, unsigned flags, size_t rbytes);
int search_range_overlapped(int device, int k, int m, int n, const void *q_d, const void *r_host, char *r_d, int dtype,
                            int64_t base, unsigned flags, nns_key *keys, nns_key *keys_tmp);
// the argument checks of every whole-call entry point (nns_search_*_ex / _topk / _multi), before any device work:
// k, m, n > 0, non-null pointers, NNS_MAX_POINTS and the k * m / k * n bounds; `where` names the entry point
int check_whole_call(const char *where, int k, int m, int n, const void *s_points, const void *r_points,
                     const int *idx_out);

// (the sum in 64 bits: a + b - 1 passes 2^31 for a point count near NNS_MAX_POINTS and a large divisor — that is how
//  a K1a plan for n = 2^31 - 2^20 once came out with a negative split count)
static inline int divup(int a, int b) { return (int)(((int64_t)a + b - 1) / b); }
static inline int64_t divup64(int64_t a, int64_t b) { return (a + b - 1) / b; }
// shard s of n refs over `shards`: contiguous ceil(n / shards) ranges, the last takes the remainder (the reference's
// split rule, core.cu:781-791; host.py shard_range mirrors it).  cnt == 0: no refs are left for shard s
struct ShardRange {
    int beg, cnt;
};
static inline ShardRange shard_range(int n, int shards, int s)
{
    const int per = divup(n, shards);
    const int64_t beg = (int64_t)s * per;
    return {(int)beg, beg + per <= n ? per : (beg < n ? (int)(n - beg) : 0)};
}

// ---- launch helpers ---------------------------------------------------------------------------------------------
// f(std::integral_constant<int, QT>{}) for the first QT of the list equal to qt; the last one takes any other value
template <int QT, int... REST, class F>
static inline int with_qt(int qt, F &&f)
{
    if constexpr (sizeof...(REST) == 0) return f(std::integral_constant<int, QT>{});
    else return qt == QT ? f(std::integral_constant<int, QT>{}) : with_qt<REST...>(qt, f);
}

// launch kern with `lds` bytes of dynamic LDS (above 48 KiB the kernel's limit is raised first)
template <typename... P, typename... A>
static inline int launch_lds(void (*kern)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, A... args)
{
    if (lds > 48 * 1024)
        NNS_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, grid, block, lds, st, args...);
    NNS_HIP(hipGetLastError());
    return NNS_OK;
}

// The grid of a lane-per-ref scan (K6, K7; 256 lanes per workgroup, one ref per lane and round): the query-tile width
// qt halves from qt0 while the fp32 query tile passes 64 KiB or qt * lds_per_query passes lds_max (0, 0: no further
// limit), then while half the tile still holds all m queries.  The refs are split so that there are about 2048
// workgroups (8 per CU), every split holds at least min_per refs and the workspace, ws_per_split bytes per split,
// stays within ws_budget; every split is whole 256-ref rounds, and the recount leaves no split empty.
struct LaneScanGrid {
    int qt, qgroups, splits, per;
};
static inline LaneScanGrid lane_scan_grid(int k, int m, int n, int qt0, size_t lds_per_query, size_t lds_max,
                                          int64_t min_per, size_t ws_per_split, size_t ws_budget)
{
    int qt = qt0;
    while (qt > 1 && ((size_t)qt * k * sizeof(float) > 64 * 1024 || qt * lds_per_query > lds_max)) qt >>= 1;
    while (qt > 1 && qt / 2 >= m) qt >>= 1;
    const int qgroups = divup(m, qt);
    int64_t splits = divup(2048, qgroups);
    const int64_t by_refs = divup64(n, min_per);
    if (splits > by_refs) splits = by_refs;
    const int64_t by_ws = (int64_t)(ws_budget / ws_per_split);
    if (splits > by_ws) splits = by_ws;
    if (splits > 65535) splits = 65535;
    if (splits < 1) splits = 1;
    const int64_t per = divup64(divup64(n, splits), 256) * 256;
    splits = divup64(n, per);
    return {qt, qgroups, (int)splits, (int)(per < n ? per : n)};
}

// The cap of every index-owned search workspace (include/nns.h): top-K's split lists, K7's per-(query, chunk) counts,
// K7m's flag bitmap of one query batch and its counts
constexpr size_t kWsBudget = (size_t)256 << 20;

// Ref-range splits of a ring-fed MFMA pass (the filter, K7m's flag pass).  One 8-wave workgroup is resident per CU, so
// the grid runs in rounds of 256 workgroups and a round that is mostly empty costs as much as a full one: choose the
// split count (up to 64, and up to max_by_mem beyond the first) that minimises rounds x (work per workgroup), i.e.
// ceil(qgroups * s / 256) / s, with a charge of 0.4 % per split (prologue, per-split outputs, merge); very few query
// groups take more splits than that scan tries, to cover all CUs.  At most one split per ring slot and 65535 (grid.y).
static inline int ring_pass_splits(int qgroups, int total_slots, int64_t max_by_mem = INT64_MAX)
{
    int splits = 1;
    double best_cost = 1e30;
    for (int sp = 1; sp <= 64 && sp <= total_slots; ++sp) {
        if (sp > 1 && sp > max_by_mem) break;
        const double cost = (double)divup(qgroups * sp, 256) / sp * (1.0 + 0.004 * sp);
        if (cost < best_cost - 1e-12) {
            best_cost = cost;
            splits = sp;
        }
    }
    if (qgroups * splits < 256) splits = divup(256, qgroups);
    if (splits > total_slots) splits = total_slots;
    if (splits > 65535) splits = 65535;
    return splits;
}

// ---- packed keys --------------------------------------------------------------
// (fp32 bits << 32) | index; distances are >= +0 so integer order == (distance,
// index) lexicographic order == V0's rule (reference core.cu:44).
__device__ __forceinline__ nns_key pack_key(float d, uint32_t idx)
{
    return ((nns_key)__float_as_uint(d) << 32) | (nns_key)idx;
}

// V0 never selects +INF or NaN (strict '>' against minSum = INFINITY).
__device__ __forceinline__ nns_key make_key(float best, int64_t idx)
{
    return (best < __builtin_inff()) ? pack_key(best, (uint32_t)idx) : (nns_key)NNS_KEY_NONE;
}

// The hit predicate of the range searches (K7, K7m: count and fill must agree on it).  NaN compares false; +INF is
// excluded explicitly (radius2 may be +INF)
__device__ __forceinline__ bool range_hit(float d, float radius2) { return d <= radius2 && d < __builtin_inff(); }

// number of set bits of `mask` below the calling lane (the slot of a lane's hit within its wave's ballot)
__device__ __forceinline__ int lanes_below(uint64_t mask)
{
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// ---- V0 arithmetic, spelled so that nothing can contract it -------------------
// reference core.cu:41-42: diff = q - r; tempSum += diff * diff  (fp32, no FMA)
__device__ __forceinline__ float v0_step(float sum, float q, float r)
{
    const float diff = __fsub_rn(q, r);
    return __fadd_rn(sum, __fmul_rn(diff, diff));
}

// ---- point element types ------------------------------------------------------------------------------------------
// The dtype of an index and of its queries (`dtype` everywhere; the C ABI's nns_plan_* take the codes as bf16_points):
// fp32, bf16 bit patterns, IEEE binary16 (fp16) bit patterns, int8 values, packed bits (one element = one 32-bit word;
// below the C-ABI entry points the dimension k counts words), uint8 values.
enum { DT_F32 = 0, DT_BF16 = 1, DT_F16 = 2, DT_I8 = 3, DT_B1 = 4, DT_U8 = 5, DT_COUNT = 6 };
// The operand form of an MFMA filter search (kFilterForms below holds a row per form): the values are the public codes of
// nns_index_filter_form.  FORM_NONE: a point type without a filter
enum { FORM_NONE = -1, FORM_F32 = 0, FORM_BF16 = 1, FORM_MIXED = 2, FORM_SPLIT = 3, FORM_F16 = 4, FORM_I8 = 5, FORM_COUNT };
// What is a fact about a point type, not about a call.  A k range of {0, 0} means "none is built".  The flag masks are
// what index_create (and, with whole_calls_check, the whole calls) refuse before the device is looked up, with the
// message "<entry point>: <text> (flags 0x..)"; check_point_flags (nns_api.hip) is the one reader.
struct PointType {
    const char *infix;             // of the C ABI's names: nns_search_<infix>_ex, nns_index_create_<infix>
    const char *name;              // in messages
    int bytes;                     // of one element
    int filter_form;               // the form the type's points take by default (fp32: operand_form chooses by flags and k;
                                   // FORM_I8: the int8 operand image, uint8 points biased by 128 in K2)
    int filter_kmin, filter_kmax;  // the MFMA filter: AUTO takes it inside this range, NNS_PATH_MFMA up to filter_kmax
    int flag_kmin, flag_kmax;      // the flag passes (NNS_RANGE_MFMA, NNS_TOPK_MFMA)
    unsigned invalid_flags;        // answered NNS_ERR_INVALID ...
    const char *invalid_text;
    unsigned unsupported_flags;    // ... and NNS_ERR_UNSUPPORTED (a type without a filter: NNS_PATH_MFMA as well)
    const char *unsupported_text;
    // The next two columns only record where today's types answer differently from one another (kept: no answer may
    // change in a refactor).  They go once those answers are made alike; a new type should not lean on them.
    bool whole_calls_check;        // the whole calls make the check too (fp16 points: index_create alone)
    bool k_checks;                 // the check also refuses NNS_PATH_MFMA beyond filter_kmax and a flag pass outside its range
};
constexpr unsigned kOperandFlags = NNS_FILTER_BF16 | NNS_FILTER_F32 | NNS_FILTER_SPLIT_EAGER;
constexpr unsigned kFlagPassFlags = NNS_RANGE_MFMA | NNS_TOPK_MFMA;
constexpr PointType kPointTypes[DT_COUNT] = {
    {"f32", "fp32", 4, FORM_SPLIT, 8, 256, 8, 256, 0, nullptr, 0, nullptr, false, false},   // (bf16-rounded operands: to 1024)
    {"bf16", "bf16", 2, FORM_BF16, 32, 1024, 32, 256, 0, nullptr, 0, nullptr, false, false},
    {"f16", "fp16", 2, FORM_F16, 32, 256, 0, 0, kOperandFlags, "the operand flags apply to fp32 points", kFlagPassFlags,
     "the range-MFMA and top-K MFMA flags are not built for fp16 points", false, false},
    {"i8", "int8", 1, FORM_I8, 32, 256, 0, 0, kOperandFlags, "the operand flags apply to fp32 points",
     kFlagPassFlags | NNS_REFS_SOA,
     "the range-MFMA and top-K MFMA flags and dimension-major refs are not built for int8 points", true, false},
    {"b1", "binary", 4, FORM_NONE, 0, 0, 0, 0, kOperandFlags, "the operand flags apply to fp32 points",
     kFlagPassFlags | NNS_REFS_SOA | NNS_RECORDS_PER_REF,
     "no MFMA filter, flag pass or dimension-major form is built for binary points", true, false},
    {"u8", "uint8", 1, FORM_I8, 32, 256, 32, 256, kOperandFlags | NNS_FILTER_I8PRE_OFF | NNS_FILTER_I8PRE_FORCE,
     "the operand flags apply to fp32 points, not to uint8 points", NNS_REFS_SOA,
     "dimension-major refs are not built for uint8 points", true, true},
};
// (a code the ABI does not define counts as bf16 points, as it did when the rules were `dtype != 0`)
inline const PointType &point_type(int dtype) { return kPointTypes[(unsigned)dtype < DT_COUNT ? dtype : DT_BF16]; }
// The points are not fp32: they are their own filter operands on the bf16 tile geometry, the operand
// flags do not apply, and the fp32-only exact kernels (K1a, K1f, K1c) are not theirs (exact_plan's `bf16`)
inline bool dt_bf16_like(int dtype) { return dtype != DT_F32; }
// uint16_t means bf16 in every overload (pt_ld1, pt_ld4, widen8, load_f, load_f4, K2); fp16 bits travel as f16_t
struct f16_t {
    uint16_t bits;
};
static_assert(sizeof(f16_t) == 2 && alignof(f16_t) == 2, "f16_t is the raw 16-bit pattern");
// binary16 -> fp32 (v_cvt_f32_f16: exact, subnormals, INF and NaN included) and the two halves of a 32-bit word
__device__ __forceinline__ float f16_widen(unsigned short b) { return (float)__builtin_bit_cast(_Float16, b); }
__device__ __forceinline__ float f16_widen_lo(unsigned w) { return f16_widen((unsigned short)(w & 0xFFFFu)); }
__device__ __forceinline__ float f16_widen_hi(unsigned w) { return f16_widen((unsigned short)(w >> 16)); }
// fp32 -> binary16 bits, round to nearest even (v_cvt_f16_f32; overflow gives INF, NaN stays NaN)
__device__ __forceinline__ unsigned f16_narrow(float v) { return __builtin_bit_cast(unsigned short, (_Float16)v); }

// point loads of the lane-per-ref scans (K1b, K6, K7): one fp32 value, or four of a 16-byte (fp32) / 8-byte (bf16, fp16) /
// 4-byte (int8, uint8) aligned row; bf16 and fp16 bits and int8 / uint8 values are widened exactly
__device__ __forceinline__ float pt_ld1(const float *p) { return *p; }
__device__ __forceinline__ float pt_ld1(const uint16_t *p) { return __uint_as_float((unsigned)*p << 16); }
__device__ __forceinline__ float4 pt_ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ float4 pt_ld4(const uint16_t *p)
{
    const uint2 v = *reinterpret_cast<const uint2 *>(p);   // 4 bf16, widened exactly
    float4 o;
    o.x = __uint_as_float(v.x << 16);
    o.y = __uint_as_float(v.x & 0xFFFF0000u);
    o.z = __uint_as_float(v.y << 16);
    o.w = __uint_as_float(v.y & 0xFFFF0000u);
    return o;
}
// int8 points travel as i8_t; every int8 value is exact in fp32
struct i8_t {
    int8_t v;
};
static_assert(sizeof(i8_t) == 1 && alignof(i8_t) == 1, "i8_t is the raw byte");
// byte e (0 .. 3) of a 32-bit word as a signed value, widened to fp32 (v_bfe_i32 + v_cvt_f32_i32: exact)
__device__ __forceinline__ float i8_widen(unsigned w, int e) { return (float)((int)(w << (24 - 8 * e)) >> 24); }
__device__ __forceinline__ float pt_ld1(const i8_t *p) { return (float)p->v; }
__device__ __forceinline__ float4 pt_ld4(const i8_t *p)
{
    const unsigned v = *reinterpret_cast<const unsigned *>(p);   // 4 int8 of a 4-byte aligned row, widened exactly
    float4 o;
    o.x = i8_widen(v, 0);
    o.y = i8_widen(v, 1);
    o.z = i8_widen(v, 2);
    o.w = i8_widen(v, 3);
    return o;
}
// uint8 points travel as u8_t; every uint8 value is exact in fp32
struct u8_t {
    uint8_t v;
};
static_assert(sizeof(u8_t) == 1 && alignof(u8_t) == 1, "u8_t is the raw byte");
// byte e (0 .. 3) of a 32-bit word as an unsigned value, widened to fp32 (v_cvt_f32_ubyte0 .. 3: one instruction, exact)
__device__ __forceinline__ float u8_widen(unsigned w, int e) { return (float)((w >> (8 * e)) & 0xFFu); }
__device__ __forceinline__ float pt_ld1(const u8_t *p) { return (float)p->v; }
__device__ __forceinline__ float4 pt_ld4(const u8_t *p)
{
    const unsigned v = *reinterpret_cast<const unsigned *>(p);   // 4 uint8 of a 4-byte aligned row, widened exactly
    float4 o;
    o.x = u8_widen(v, 0);
    o.y = u8_widen(v, 1);
    o.z = u8_widen(v, 2);
    o.w = u8_widen(v, 3);
    return o;
}
__device__ __forceinline__ float pt_ld1(const f16_t *p) { return f16_widen(p->bits); }
__device__ __forceinline__ float4 pt_ld4(const f16_t *p)
{
    const uint2 v = *reinterpret_cast<const uint2 *>(p);   // 4 fp16, widened exactly
    float4 o;
    o.x = f16_widen_lo(v.x);
    o.y = f16_widen_hi(v.x);
    o.z = f16_widen_lo(v.y);
    o.w = f16_widen_hi(v.y);
    return o;
}

// binary points travel as b1_t: one raw word of 32 bits, bit t of a point = (word[t / 32] >> (t % 32)) & 1.  A word is
// never widened: the scans move it as `unsigned` (tile_word_t, v0_lane_chains' b1_t overload)
struct b1_t {
    uint32_t w;
};
static_assert(sizeof(b1_t) == 4 && alignof(b1_t) == 4, "b1_t is the raw 32-bit word");

// f(PointTag<T>{}) for the element type T of dtype, in the style of with_qt: the one place a launcher turns the dtype
// into a kernel's element type.  `default` is bf16 because a code the ABI does not define has always counted as bf16
// points (point_type); it stands where DT_BF16 stood in the chains this replaces, so that the kernels are instantiated,
// and laid out in the code object, in the order they always were
template <typename T>
struct PointTag {
    using type = T;
};
template <class F>
static inline int with_point_type(int dtype, F &&f)
{
    switch (dtype) {
    case DT_B1: return f(PointTag<b1_t>{});
    case DT_U8: return f(PointTag<u8_t>{});
    case DT_I8: return f(PointTag<i8_t>{});
    case DT_F16: return f(PointTag<f16_t>{});
    default: return f(PointTag<uint16_t>{});
    case DT_F32: return f(PointTag<float>{});
    }
}
static_assert(sizeof(float) == kPointTypes[DT_F32].bytes && sizeof(uint16_t) == kPointTypes[DT_BF16].bytes &&
                  sizeof(f16_t) == kPointTypes[DT_F16].bytes && sizeof(i8_t) == kPointTypes[DT_I8].bytes &&
                  sizeof(b1_t) == kPointTypes[DT_B1].bytes && sizeof(u8_t) == kPointTypes[DT_U8].bytes,
              "the table's element bytes are the tag types' sizes");

__device__ __forceinline__ unsigned pt_ld1(const b1_t *p) { return p->w; }
// The element type of the LDS query tile of a lane-per-ref scan: the widened fp32 value, or for b1_t the raw word.  The
// tile is declared float for every point type; a b1_t tile is written and read as unsigned only (a float move may
// canonicalise a word that happens to be a NaN pattern)
template <typename T>
using tile_word_t = std::conditional_t<std::is_same_v<T, b1_t>, unsigned, float>;

// ---- the lane-per-ref scan core (K1b, K6, K7) ----------------------------------------------------------------------
// One lane holds one ref row rj; the fp32 query tile sq[QT][k] sits in LDS and is read by broadcast.  sum[u] = V0's
// distance of query u to the ref: one t-ascending v0_step chain per query (VEC 4: a float4 of the row per step, k % 4 == 0
// and the row 16- / 8-byte aligned; VEC 1: one value per step, the loop unrolled UNROLL times).
template <int QT, int VEC, int UNROLL, typename T>
__device__ __forceinline__ void v0_lane_chains(int k, const float *sq, const T *rj, float (&sum)[QT])
{
#pragma unroll
    for (int u = 0; u < QT; ++u) sum[u] = 0.0f;
    if (VEC == 4) {
        for (int t = 0; t < k; t += 4) {
            const float4 rv = pt_ld4(rj + t);
#pragma unroll
            for (int u = 0; u < QT; ++u) {
                const float4 qv = *reinterpret_cast<const float4 *>(&sq[u * k + t]);   // broadcast
                float s = sum[u];
                s = v0_step(s, qv.x, rv.x);
                s = v0_step(s, qv.y, rv.y);
                s = v0_step(s, qv.z, rv.z);
                s = v0_step(s, qv.w, rv.w);
                sum[u] = s;
            }
        }
    } else {
#pragma unroll UNROLL
        for (int t = 0; t < k; ++t) {
            const float rv = pt_ld1(rj + t);
#pragma unroll
            for (int u = 0; u < QT; ++u) sum[u] = v0_step(sum[u], sq[u * k + t], rv);
        }
    }
}

// The same scan for binary points (b1_t): k counts 32-bit words, sq holds the QT query rows as raw words.  V0's distance
// of 0 / 1 values is the Hamming distance (every term fl(fl(q - r)^2) is 0 or 1, every partial sum an integer below
// 2^24: k <= 16384 words = 2^19 bits), so per word one xor and one popcount that adds into an integer accumulator
// (v_xor_b32 + v_bcnt_u32_b32), and one exact v_cvt_f32_u32 per (query, ref) at the end.  VEC 4: 16 bytes of the ref
// row per step (k % 4 == 0, rows 16-byte aligned), the query words by one broadcast ds_read_b128; VEC 1: one word.
// acc + popcount(x) in the one instruction that does both.  Spelled as asm: from `acc += __popc(x)` the compiler (ROCm 7.2)
// reassociates the sums of a step into popcounts onto 0 plus v_add3_u32, 2.5 instead of 2 instructions per word.
__device__ __forceinline__ unsigned popc_add(unsigned x, unsigned acc)
{
    unsigned out;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(out) : "v"(x), "v"(acc));
    return out;
}

template <int QT, int VEC, int UNROLL>
__device__ __forceinline__ void v0_lane_chains(int k, const float *sq, const b1_t *rj, float (&sum)[QT])
{
    const unsigned *sw = reinterpret_cast<const unsigned *>(sq);
    unsigned acc[QT];
#pragma unroll
    for (int u = 0; u < QT; ++u) acc[u] = 0u;
    if (VEC == 4) {
        for (int t = 0; t < k; t += 4) {
            const uint4 rv = *reinterpret_cast<const uint4 *>(rj + t);
#pragma unroll
            for (int u = 0; u < QT; ++u) {
                const uint4 qv = *reinterpret_cast<const uint4 *>(&sw[u * k + t]);   // broadcast
                unsigned a = acc[u];
                a = popc_add(qv.x ^ rv.x, a);
                a = popc_add(qv.y ^ rv.y, a);
                a = popc_add(qv.z ^ rv.z, a);
                a = popc_add(qv.w ^ rv.w, a);
                acc[u] = a;
            }
        }
    } else {
#pragma unroll UNROLL
        for (int t = 0; t < k; ++t) {
            const unsigned rv = rj[t].w;
#pragma unroll
            for (int u = 0; u < QT; ++u) acc[u] += __popc(sw[u * k + t] ^ rv);   // (plain C: an asm statement keeps the loop from unrolling)
        }
    }
#pragma unroll
    for (int u = 0; u < QT; ++u) sum[u] = (float)acc[u];
}

// K6 / K7's VEC 1 unroll: what the compiler chose for their loops before they shared v0_lane_chains (through the
// helper it left QT = 16 rolled, 10 % slower at k = 3).  K1b's grid-stride scan passes 1: it was never unrolled.
template <int QT>
constexpr int kLaneScanUnroll = QT >= 8 ? 2 : QT == 4 ? 4 : 8;

// the query tile of K6 / K7: queries q0 .. q0 + QT - 1 widened to fp32 into sq[QT][k] (b1_t: the raw words), zeros past m
template <int QT, int THREADS, typename T>
__device__ __forceinline__ void load_query_tile(float *sq, const T *q, int q0, int m, int k)
{
    for (int e = threadIdx.x; e < QT * k; e += THREADS) {
        const int u = e / k, t = e - u * k;
        reinterpret_cast<tile_word_t<T> *>(sq)[e] = q0 + u < m ? pt_ld1(q + (size_t)(q0 + u) * k + t) : tile_word_t<T>(0);
    }
}

// ---- the top-K lists of a workgroup (K6's scan, K6m's selection) ---------------------------------------------------
constexpr int kTopkThreads = 256;
constexpr int kTopkQueue = 512;                    // queue capacity per query (keys)
constexpr int kTopkFlushAt = kTopkQueue - kTopkThreads;   // a queue this full is flushed before the next round

// number of entries of the sorted row a[0..len) below v (strict), or at most v (or_equal)
__device__ __forceinline__ int tk_rank(const nns_key *a, int len, nns_key v, bool or_equal)
{
    int lo = 0, hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const nns_key x = a[mid];
        if (x < v || (or_equal && x == v)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The flush of K6's scan and K6m's selection (topk_mfma.hip), called by all kTopkThreads threads of the workgroup after a
// barrier that follows the last append: the QT queues (qcnt[u] keys each) are sorted (bitonic, in LDS), merged by rank into
// the other half of the ping-pong lists [2][QT][kn], `cur` flips, thr[u] becomes list u's kn-th key and the counts are
// zeroed.  Returns behind a barrier.  Keys are unique within a search, so every rank below is exact.
template <int QT>
__device__ __forceinline__ void topk_flush(nns_key *lists, nns_key *queue, int *qcnt, int kn, int &cur, nns_key (&thr)[QT])
{
    const int tid = threadIdx.x;
    int maxc = 0;
#pragma unroll
    for (int u = 0; u < QT; ++u) maxc = qcnt[u] > maxc ? qcnt[u] : maxc;
    if (maxc == 0) return;   // (workgroup-uniform: nothing changes qcnt between the barrier and here)
    int P = 1;
    while (P < maxc) P <<= 1;   // <= kTopkQueue
    nns_key *src = lists + cur * QT * kn, *dst = lists + (cur ^ 1) * QT * kn;
    for (int e = tid; e < QT * P; e += kTopkThreads) {
        const int u = e / P, i = e - u * P;
        if (i >= qcnt[u]) queue[u * kTopkQueue + i] = NNS_KEY_NONE;
    }
    for (int e = tid; e < QT * kn; e += kTopkThreads) dst[e] = NNS_KEY_NONE;
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int e = tid; e < QT * (P >> 1); e += kTopkThreads) {
                const int u = e / (P >> 1), i = e - u * (P >> 1);
                const int lo = 2 * stride * (i / stride) + (i % stride), hi = lo + stride;
                nns_key *qq = queue + u * kTopkQueue;
                const nns_key a = qq[lo], b = qq[hi];
                const bool up = (lo & size) == 0;
                if ((a > b) == up) {
                    qq[lo] = b;
                    qq[hi] = a;
                }
            }
            __syncthreads();
        }
    // rank merge: an old entry goes before equal queue entries (there are none: keys are unique)
    for (int e = tid; e < QT * kn; e += kTopkThreads) {
        const int u = e / kn, i = e - u * kn;
        const nns_key a = src[e];
        if (a == NNS_KEY_NONE) continue;
        const int rk = i + tk_rank(queue + u * kTopkQueue, qcnt[u], a, false);
        if (rk < kn) dst[u * kn + rk] = a;
    }
    const int qtake = P < kn ? P : kn;   // a queue entry at position >= kn cannot land in the first kn
    for (int e = tid; e < QT * qtake; e += kTopkThreads) {
        const int u = e / qtake, i = e - u * qtake;
        if (i >= qcnt[u]) continue;
        const nns_key b = queue[u * kTopkQueue + i];
        const int rk = i + tk_rank(src + u * kn, kn, b, true);
        if (rk < kn) dst[u * kn + rk] = b;
    }
    __syncthreads();
    cur ^= 1;
#pragma unroll
    for (int u = 0; u < QT; ++u) thr[u] = dst[u * kn + kn - 1];
    __syncthreads();   // every thread has read the counts and thresholds before they change
    if (tid < QT) qcnt[tid] = 0;
    __syncthreads();
}

// LDS-DMA (global_load_lds_*): 64 lanes x {16, 4} bytes from per-lane global addresses to
// LDS at M0 + lane * size, no VGPR destination.  Inline asm on purpose: through the
// builtin, hipcc (ROCm 7.2) treats every later ds_read as possibly aliasing the
// in-flight DMA and drains it with s_waitcnt vmcnt(0) right after the issue.  The asm
// form is invisible to that pass; completion is tracked by OUR vmcnt waits + the slot
// barrier.  M0 is compiler-reserved: saved and restored inside the same statement.
__device__ __forceinline__ void dma16(const void *g, unsigned lds_byte)
{
    lds_byte = __builtin_amdgcn_readfirstlane(lds_byte);   // wave-uniform by construction: keep it scalar
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(g), "s"(lds_byte)
                 : "memory");
}
__device__ __forceinline__ void dma4(const void *g, unsigned lds_byte)
{
    lds_byte = __builtin_amdgcn_readfirstlane(lds_byte);
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                 "global_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(g), "s"(lds_byte)
                 : "memory");
}

// ---- tile-image geometry (K2 output, K3 input) ---------------------------------
// A "block" is 32 points.  Its image is [KT/8][2][32][4] floats:
//   img[b][h][i][e] = value(point i, dim 8b + 4h + e)
// i.e. exactly the order in which the 64 lanes of a wave (lane = 32h + i) read
// float4 #b, so one ds_read_b128 / global_load_dwordx4 per lane is lane-linear
// (1 KiB contiguous per wave-instruction, bank-conflict free), and the four
// floats are the operands of MFMA k-steps 4b..4b+3 for that lane
// (v_mfma_f32_32x32x2_f32: lane supplies A[i = lane&31][k = lane>>5]).
constexpr int kBlockPts = 32;

// Blocks and ring slots of the filter (filter_main's constants, filter_plan's paddings).  A block of 32 refs is spb 1 KiB
// fragment steps, a ring slot sps steps (32; the lazy operators' hi-only slots 16).  A block that divides the slot: one
// slot, sps / spb whole blocks.  A deeper block straddles slots with a super-period of lcm(spb, 32) steps: 64 steps
// (1024-deep): 2 slots = 1 block; 48 (768-deep): 3 slots = 2 blocks; 40 (640-deep): 5 = 4; 24 (384-deep): 3 = 4.
struct RingGeom {
    bool deep;                     // the block does not divide the slot
    int slots, blocks, slot_refs;  // of a super-period; 32 * blocks: the norms that travel with a slot, the refs' padding unit
};
__host__ __device__ constexpr RingGeom ring_geom(int spb, int sps = 32)
{
    const bool deep = sps % spb != 0;
    const int g = spb % 32 == 0 ? 32 : (spb % 16 == 0 ? 16 : (spb % 8 == 0 ? 8 : 1));
    const int blocks = deep ? 32 / g : sps / spb;
    return {deep, deep ? spb / g : 1, blocks, 32 * blocks};
}

// The bf16 filter at KT 128 / 256 / 512 runs v_mfma_f32_16x16x32_bf16 on 16x16 tiles (the chip clocks ~14 % higher on
// it under load than on the 32x32x16 form).  That fixes the bf16 tile-image order, 1 (prep_kernels.hip), and the four
// lanes a query's candidate lists live on (FilterGeom.lpq, finalize.hip).
constexpr int kBf16ImageOrder = 1;

// the eager split operators' workgroup and ring slot (OpSplitT; filter_plan asserts them), shared by K7m's flag kernel
constexpr int kSplitWaves = 8;        // waves per workgroup: two per SIMD
constexpr int kSplitSlotSteps = 32;   // 1 KiB fragment steps per ring slot
// 32-query blocks per wave of K7m's flag kernel for bf16 points (range_flag16_kernel): OpBF16K128 / OpBF16's, so that the
// plan's query groups are filter_plan's
constexpr int kFlag16QB = 2;
// a chunk of K7m's evaluation and of K6m's selection is whole steps of this many flag words
constexpr int kRmChunkWords = 64;

// A v_mfma_f32_16x16x32_bf16 operand out of a 32-point block in the 32x32x16 operand order (K2 forms 2 and 3: 16-dim
// fragment s holds, at lane 32 hl + p, dims 16 s + 8 hl .. + 7 of point p).  Lane l = 16 g + i of the operand of point
// tile t (points 16 t + i), k-step ks wants dims 32 ks + 8 g .. + 7: the 16 bytes at fragment 2 ks + (g >> 1), lane
// 32 (g & 1) + 16 t + i.  Returned as a 16-byte index into the block's fragments; `parts` = 1: fragments of one part
// back to back (form 3's hi or lo region), 2: hi and lo interleaved per 16-dim step (form 2, the query image), `part`
// then picks hi (0) or lo (1).  (tools/lazy16_gather_check.cpp checks it against the order-1 definition of
// prep_kernels.hip and counts the banks of every ds_read_b128 lane group.)
__host__ __device__ constexpr int lazy16_gather(int lane, int t, int ks, int parts = 1, int part = 0)
{
    const int g = lane >> 4, i = lane & 15;
    return ((2 * ks + (g >> 1)) * parts + part) * 64 + 32 * (g & 1) + 16 * t + i;
}

// The int8 pre-pass's ring (OpI8Pre, filter_mfma.hip): kI8PreRingDepth slots, a slot's DMA issued kI8PreAhead intervals
// before the interval that reads it, and a workgroup barrier only at the intervals s with s % kI8PreGroup == 0.
// Between two barriers a wave is anywhere inside its group g: it reads slots gG .. gG + G (an interval reads its own slot
// and, for its last fragments' prefetch and the next tile's seeds, the next one) and its DMA writes slots gG + AHEAD ..
// gG + G - 1 + AHEAD.  The barrier that opens group g confirms slots gG + 1 .. gG + G with the counted wait
// vmcnt((AHEAD - G - 1) pieces per wave): the youngest of them must have been issued (G < AHEAD), and the leader's
// youngest write must not reach the laggard's oldest read one ring turn on (AHEAD + G - 1 < depth).
// (tools/pre_cadence_check.cpp brute-forces the protocol against this closed form.)
#ifndef NNS_F_PRE_AHEAD
#define NNS_F_PRE_AHEAD 8
#endif
#ifndef NNS_F_PRE_GROUP
#define NNS_F_PRE_GROUP 4
#endif
constexpr int kI8PreRingDepth = 16;
constexpr int kI8PreAhead = NNS_F_PRE_AHEAD;
constexpr int kI8PreGroup = NNS_F_PRE_GROUP;
__host__ __device__ constexpr bool pre_cadence_ok(int depth, int ahead, int group)
{
    return group >= 1 && group < ahead && ahead + group <= depth;
}

struct FilterGeom {
    int dtype;            // the points' type (DT_*): what K2 and K5 read
    int form;             // the operand form the plan grants (FORM_*, kFilterForms): SPLIT only at the depths split_depth names
    int lpq;              // lanes (= private candidate lists) per query and split: 2, or 4 with 16x16 tiles
    int lazy;             // FORM_SPLIT: the lazy schedule (OpLazySplitT: cross products only on tiles near the threshold)
    int lazy_img;         // FORM_SPLIT: the ref image is in the lazy layout (hi fragments | lo fragments; K2 form 3)
    int kt;               // K of the tile (k padded up with zeros)
    int spb;              // 1 KiB fragment steps per 32-ref block of the tile image (the operator's kSPB; a lazy search:
                          // its eager twin's — hi and lo fragments — which is how the image is sized either way)
    int qb;               // 32-query blocks per wave (kQB)
    int waves;            // waves per workgroup (kNW)
    int qw;               // queries per workgroup: 32 * qb * waves
    int m_pad;            // queries padded to the workgroup's query count
    int n_pad;            // refs padded to a whole ring slot
    int total_slots;      // n_pad / (32 * kSlotBlocks)
    int splits;           // grid.y: contiguous ref ranges
    int slots_per_split;
    int qgroups;          // grid.x
    int slot_pts;         // refs per ring slot
    int share_thr;        // short ref streams: a query's lanes share their record thresholds
    int tile_rec;         // short ref streams: candidate entries are (tile minimum, first ref of the lane's rows of that
                          // tile) — K5 evaluates all of the lane's rows — instead of (score, ref).  1: appended behind the
                          // threshold test (16 x 16 tiles); 2: the lane's two best tiles + its third-best minimum,
                          // tracked branch-free (32 x 32 tiles)
};

// One candidate of the filter: score s = |y'|^2 - 2 x'.y' and shard-local ref index.
struct __attribute__((aligned(8))) CandEntry {
    float s;
    int j;
};
// capacity of one lane's private candidate list (per split, query, lane half).  The list
// is a RING: a lane collects ~ln(refs it sees) records, and when more than kCandCap were
// appended (monotone inputs) the oldest entry is overwritten — provably harmless when its
// score is above the lane's current threshold (thresholds only shrink), otherwise the
// overflow bit is set and the query is re-ranked by the exact scan instead.
constexpr int kCandCap = 64;                 // power of two
constexpr int kCandOverflow = 1 << 30;       // bit of the per-list count word
constexpr int kCandCountMask = kCandOverflow - 1;

// tau(a) = c0 + c1 * max(a + x2, 0): the margin within which a filter score cannot be
// ordered against V0's fp32 distances (derivation: finalize.hip).  Shared by K3/K4 (which
// widen it by 0.2 % so their candidate sets are supersets) and K5.
struct TauConsts {
    float c0, c1, x2;
};

// The tau mode of a filter search (FilterArgs::tau_mode, K5's tau_mode; nns_tau_consts takes the values over the ABI):
// fp32 operands, bf16 points (operands exact), fp32 points ROUNDED to bf16 operands, fp32 points as SPLIT bf16 operands
// (hi + lo, three products: OpSplitT), fp16 points (operands exact) on v_mfma_f32_16x16x32_f16:
// two binary16 values multiply exactly in fp32 (11 + 11 significand bits), so mode 1's formula — exact products, the
// order-free accumulation model at kMode4AddUlps u per add, no centring — holds as it stands ("fp16 points")
constexpr double kMode4AddUlps = 2.0;
enum { TAU_F32 = 0, TAU_BF16 = 1, TAU_MIXED = 2, TAU_SPLIT = 3, TAU_F16 = 4 };
// The chains of nns_selftest_mfma (its own numbering over the ABI: 4 is the lazy order there): fp32, bf16 32x32x16, bf16
// 16x16x32, the split chain, the split chain in the lazy filter's order, f16 16x16x32, i8 16x16x64
enum { ST_F32 = 0, ST_BF16 = 1, ST_BF16_T16 = 2, ST_SPLIT = 3, ST_LAZY = 4, ST_F16 = 5, ST_I8 = 6 };

// What is a fact about an operand form (FORM_*), one row each; FilterGeom::form indexes it (DESIGN, "The operand forms").
// I8 has no tau mode of its own: its scores are exact integers, so TAU_BF16's margin is a valid one.
enum { K2_F32, K2_BF16, K2_I8 };   // K2's three image kernels: fp32 points (centred), 16-bit points, 8-bit points
struct FilterForm {
    const char *name;     // in messages
    int img_bytes;        // of one dimension of a point's tile-image row
    int tau_mode;         // TAU_*: launch_filter and K5 agree on it
    int bf16;             // nns_plan_filter's field 1: the bf16 tiles' geometry
    int ladder[8];        // the tile depths, ascending, 0 behind the last: a plan takes the first that holds k
    int k2_image;         // K2_*
    int k2_form;          // K2_F32: launch_prep_image's form (the refs of a lazy-layout index take 3 instead of 2)
};
constexpr FilterForm kFilterForms[FORM_COUNT] = {
    {"fp32", 4, TAU_F32, 0, {16, 32, 64, 128, 256}, K2_F32, 0},
    {"bf16", 2, TAU_BF16, 1, {128, 256, 384, 512, 640, 768, 1024}, K2_BF16, 0},
    {"mixed", 2, TAU_MIXED, 1, {128, 256, 384, 512, 640, 768, 1024}, K2_F32, 1},
    {"split", 4, TAU_SPLIT, 0, {16, 32, 64, 128, 256}, K2_F32, 2},
    {"fp16", 2, TAU_F16, 1, {128, 256}, K2_BF16, 0},
    {"int8", 1, TAU_BF16, 1, {256}, K2_I8, 0},
};

// ---- sizes of the images and what sits beside them (nns_api.hip allocates, K2 and the filter address) -----------------
// one point of a tile image
inline size_t img_row_bytes(const FilterGeom &g) { return (size_t)g.kt * kFilterForms[g.form].img_bytes; }
// The filter's ring DMA runs up to three slots (32 KiB of image, slot_pts norms each) past the last one without a
// bounds branch: images and norm arrays carry that much padding (+ the over-read of a 128-norm piece)
inline size_t img_bytes(const FilterGeom &g, int pts_pad) { return (size_t)pts_pad * img_row_bytes(g) + 3 * 32768 + 4096; }
inline size_t norm_bytes(const FilterGeom &g, int pts_pad) { return ((size_t)pts_pad + 3 * g.slot_pts + 256) * sizeof(float); }
// The int8 pre-pass's operands sit behind the image they go with, in the same allocation, at these byte offsets from the
// image's start.  Refs: the int8 region (128 bytes per ref; its ring runs up to 16 slots of 8 KiB past the end), then one
// i32 seed per ref (+ 16 slots of 64).  Queries: the q8 image (128 bytes per query), then one fp32 bound per query.
struct I8PreLayout {
    size_t img8, aux, end;   // the int8 image; the seeds (refs) or bounds (queries); the end of the allocation
};
inline I8PreLayout i8pre_layout(const FilterGeom &g, int pts_pad, bool refs)
{
    const size_t img8 = img_bytes(g, pts_pad), aux = img8 + (size_t)pts_pad * 128 + (refs ? 16 * 8192 : 0);
    return {img8, aux, aux + (refs ? ((size_t)pts_pad + 16 * 64) * sizeof(int) : (size_t)pts_pad * sizeof(float))};
}
__host__ __device__ inline TauConsts tau_consts(int kt, float qnorm2, float ymax2, int mode)
{
    const bool bf16 = mode != TAU_F32;
    const double u = 5.9604644775390625e-08;   // 2^-24
    const double X2 = (double)qnorm2 * (1.0 + 4.0 * u);
    const double Y2 = (double)ymax2 * (1.0 + 4.0 * u);
    const double X = sqrt(X2), Y = sqrt(Y2);
    const double gk = (kt + 2) * u / (1.0 - (kt + 2) * u);   // V0's own rounding (k+1 per term)
    double e3, e2;
    if (mode == TAU_SPLIT) {
        // Split operands (derivation: DESIGN.md, "Exactness"), a = u_b = 2^-8: v = h + l + d with h = rn_bf16(v),
        // l = rn_bf16(v - h), |h| <= (1 + a)|v|, |l| <= a (1 + a)|v|, |d| <= a^2 |v|.  qh.rh + qh.rl + ql.rh drops
        // qh.d_r + ql.rl + ql.d_r + d_q.v, at most a^2 (3 + 4a + 2a^2) |x'_t v_t| <= 3 * 2^-16 (1 + 2^-6) |x'_t v_t|,
        // summed <= 3 * 2^-15 (1 + 2^-6) X Y (v = -2 y').  Products exact in fp32; the seeded accumulation of
        // 3 kt / 16 MFMAs = 3 kt products under the 32x32x16 model above (2u per add) on
        // sum |products| <= (1 + a)^2 (1 + 2a) sum |x'_t v_t| <= (1 + 2^-5) 2 X Y.  Absolute floor: an operand part below 2^-126 (subnormal: flushed or
        // not by the MFMA) is off by < 2^-126 — 2^-124 (|x'_t| + |v_t|) per element covers all three products, summed
        // <= 2^-124 sqrt(kt) (X + 2 Y) — and a product or an add with a result below 2^-126 loses < 2^-126 each.
        const double na = 3.0 * kt + 3.0 * (kt / 16) + 2.0;
        const double gs = 2.0 * na * u / (1.0 - 2.0 * na * u);
        const double et = 3.0 * 0x1p-15 * (1.0 + 0x1p-6) * X * Y;
        const double ef = 0x1p-124 * sqrt((double)kt) * (X + 2.0 * Y) + (7.0 * kt + 4.0) * 0x1p-126;
        e3 = gs * (Y2 + (1.0 + 0x1p-5) * 2.0 * X * Y) + 2.0 * u * Y2 + et + ef;
        e2 = 2.5 * u * (X + Y) * (X + Y);   // x' = fl(x - c), y' = fl(y - c), as on the fp32 path
    } else if (!bf16) {
        // fp32 MFMA = k-ordered fmaf chain of kt steps seeded with the rounded norm
        e3 = gk * (Y2 + 2.0 * X * Y) + 2.0 * u * Y2;
        e2 = 2.5 * u * (X + Y) * (X + Y);   // x' = fl(x - c), y' = fl(y - c)
    } else {
        // bf16 products are exact in fp32; the accumulation order/rounding inside
        // v_mfma_f32_32x32x16_bf16 is not documented: allow 2u per add, kt + kt/16 adds
        const double pa = mode == TAU_F16 ? kMode4AddUlps : 2.0;   // allowance per add, in u
        const double gf = pa * (kt + kt / 16 + 2) * u / (1.0 - pa * (kt + kt / 16 + 2) * u);
        e3 = gf * (Y2 + 2.0 * X * Y) + 2.0 * u * Y2;
        e2 = 0.0;                            // no centring on the bf16 path
        if (mode == TAU_MIXED) {
            // operands x^ = rn_bf16(x'), y^ = rn_bf16(y') with |x^ - x'| <= 2^-8 |x'| (8-bit significand):
            // |x^.y^ - x'.y'| <= (2 * 2^-8 + 2^-16) sum |x'_t||y'_t| <= 2^-7 (1 + 2^-9) X Y, doubled by the
            // factor -2 of the score; plus the centring term of the fp32 path (x' = fl(x - c)), and the
            // accumulation bound above on the slightly larger rounded magnitudes
            e3 = e3 * (1.0 + 0x1p-6) + 0x1p-6 * (1.0 + 0x1p-8) * X * Y;
            e2 = 2.5 * u * (X + Y) * (X + Y);
        }
    }
    const double c1 = 2.0 * gk / (1.0 - gk) * 1.001;
    // er: the fp32 rounding of the THRESHOLD SUM itself.  K5 forms fl(a + tau_fl(a)) and the filter
    // fl(t + fl(1.002 tau_fl(t))): one rounding of a sum whose magnitude is set by the score, not by tau —
    // |a| <= max(X^2, Y^2 + 2XY) + e3 <= (X + Y)^2 + e3 — so it can pull the threshold down by u (|a| + tau),
    // up to 1 / (2 (K + 2)) of tau itself (2.8 % at K = 16): more than the 0.1 % factors below absorb.  It gets a
    // term of its own (2u instead of u: the evaluation of tau_fl — three more roundings, relative — and the
    // rounding of the term itself ride on the spare u and on the 1.001 factors; finalize.hip, "fp32 evaluation").
    const double er = 2.0 * u * ((X + Y) * (X + Y) + e3 + e2);
    const double c0 = (2.0 + c1) * (e3 + e2) * 1.001 + er + 1e-30;
    TauConsts t;
    t.c0 = (float)(c0 * (1.0 + 1e-6));
    t.c1 = (float)(c1 * (1.0 + 1e-6));
    t.x2 = (float)(X2 * (1.0 + 1e-6));
    return t;
}

// B of the lazy split filter (OpLazySplitT): an upper bound, per query, on s_hh - s_3 — how far the finished
// three-product score of a (query, ref) pair can lie BELOW the score its accumulator held after the hi-hi products
// alone — plus the rounding of the kernel's fl(thr + B).  A tile whose hi-hi minimum is above fl(thr + B) has no
// three-product score within thr.  Same X, Y, a = 2^-8 and operand bounds as tau_consts' mode 3 (v = -2 y'):
//   cross products  |qh.rl + ql.rh| <= sum (|qh_t||rl_t| + |ql_t||rh_t|) <= 2a (1 + a)^2 sum |x'_t v_t| <= 2a (1 + a)^2 2XY;
//   their accumulation: 2 kt products in 2 kt / 16 MFMAs continue the accumulator, 2u per add (the order-free model of
//     mode 3) on partial sums of magnitude <= Y^2 + sum |products| <= Y^2 + (1 + 2^-5) 2XY;
//   the absolute floor of mode 3 for operand parts, products and adds below 2^-126 (all three products' worth);
//   fl(thr + B): one rounding at the magnitude of the score, |thr + B| <= (X + Y)^2 (1 + small) — 2u (X + Y)^2 as
//     tau_consts' er term (the spare u covers tau, B and e3 riding on thr).
// (The hi-hi partial's own accumulation error is in neither s_hh nor s_3 twice: both are values of the same accumulator.)
__host__ __device__ inline float split_lazy_bound(int kt, float qnorm2, float ymax2)
{
    const double u = 5.9604644775390625e-08;   // 2^-24
    const double a = 0x1p-8;
    const double X2 = (double)qnorm2 * (1.0 + 4.0 * u);
    const double Y2 = (double)ymax2 * (1.0 + 4.0 * u);
    const double X = sqrt(X2), Y = sqrt(Y2);
    const double cross = 2.0 * a * (1.0 + a) * (1.0 + a) * 2.0 * X * Y;
    const double nb = 2.0 * kt + 2.0 * (kt / 16) + 2.0;
    const double gb = 2.0 * nb * u / (1.0 - 2.0 * nb * u);
    const double acc = gb * (Y2 + (1.0 + 0x1p-5) * 2.0 * X * Y);
    const double ef = 0x1p-124 * sqrt((double)kt) * (X + 2.0 * Y) + (7.0 * kt + 4.0) * 0x1p-126;
    const double er = 2.0 * u * ((X + Y) * (X + Y) + cross + acc + ef);
    return (float)((cross + acc + ef + er + 1e-30) * (1.0 + 1e-6));
}

__host__ __device__ inline float tau_of(const TauConsts &t, float a)
{
    const float d = a + t.x2;
    return t.c0 + t.c1 * (d > 0.0f ? d : 0.0f);
}

// The record threshold a filter lane derives from a score a it has seen: a + 1.002 tau(a) (a hair
// wider than K5's own tau so that the lists are supersets of what K5 needs).  Monotone in a, so the
// threshold of a minimum is the minimum of the thresholds.  (The filter's slow path, tighten, spells the
// same expression with its constants in registers.)
__host__ __device__ inline float record_threshold(const TauConsts &t, float a)
{
    const float d = a + t.x2;
    return a + (t.c0 + t.c1 * (d > 0.0f ? d : 0.0f)) * 1.002f;
}

// K7m's flag threshold of a query (range_mfma.hip): a ref whose V0 distance is <= radius2 has a split-bf16 score
// (tau mode 3) <= this value.  With a = fl(radius2 - |x'|^2): fl(a + 1.002 tau(a)), the filter's record threshold at a,
// plus 2^-22 (radius2 + |x'|^2) for the roundings of the subtraction and of the two sums, which are relative to
// max(radius2, |x'|^2) — a magnitude tau's own rounding term (sized for scores, <= (X + Y)^2) does not cover once the
// radius is far larger than the cloud.  Monotone in radius2.  Derivation: DESIGN section 4, "K7m".
//
// mode 1 (bf16 points, range_flag16_kernel): the same form over tau_consts' mode 1 — exact operands and products, the
// order-free accumulation model, no centring (e2 = 0) — with qnorm2 = K2's uncentred |x|^2 and ymax2 the refs' largest
// |y|^2.  Monotone in radius2 as well.  DESIGN section 4, "K7m", "bf16 points".
__host__ __device__ inline float range_threshold(int kt, float qnorm2, float ymax2, float radius2, int mode = TAU_SPLIT)
{
#pragma clang fp contract(off)
    const TauConsts t = tau_consts(kt, qnorm2, ymax2, mode);
    const float a = radius2 - qnorm2;
    const float thr = record_threshold(t, a);
    return thr + 0x1p-22f * (radius2 + qnorm2);
}

// K7m's flag threshold of a uint8 query (range_mfma.hip, RmU8Tile).  Score and distance are exact integers there: with
// x' = x - 128, y' = y - 128 the score is s = |y'|^2 - 2 x'.y', |s| < 2^24, and V0's distance is d = |x'|^2 + s, an integer
// of at most 16 646 400 < 2^24.  So d <= radius2  <=>  d <= R := floor(min(radius2, 2^24)), an integer in 0 .. 2^24.
// qnorm2 = |x'|^2 is an integer in 0 .. 2^22, so R - qnorm2 is an integer in -2^22 .. 2^24: the fp32 subtraction is exact,
// and s <= thr  <=>  s + |x'|^2 <= R  <=>  d <= radius2.  No margin: a block is flagged if and only if it holds a hit.
// radius2 >= 0 and not NaN (the callers' check); +INF is the callers' case (thr = -INF and a filled row).
__host__ __device__ inline float range_threshold_u8(float qnorm2, float radius2)
{
#pragma clang fp contract(off)
    return floorf(fminf(radius2, 0x1p24f)) - qnorm2;
}

// tau(a) of K1f, the vector-ALU filter of k <= 3 (exact_kernels.hip, lowdim_filter_kernel), in fp32, rounded up everywhere.
// Its score is an FMA chain of 2K steps (K for the norm of y' = fl(r - c), K for -2 x'.y' on top of it), so the relative
// part is tau_consts' model at kt = 2K <= 8 with (X + Y)^2 <= 2 (X^2 + Y^2): c0 <= 62.2 u (X^2 + Y^2), c1 <= 20.1 u.
// x2, y2 >= X^2, Y^2 (the kernel passes its FMA-chain norms times 1.00001f).
// The absolute part: a rounding whose RESULT lies below FLT_MIN is off by up to half a subnormal ulp, 2^-150, however
// small the operands — a bound no relative term gives once the squares are subnormal (at the smallest scales the
// relative part rounds to 0).  Additions and subtractions with a subnormal result are exact, so the centrings
// x' = fl(q - c), y' = fl(r - c) and V0's adds add nothing; what does is every FMA of the two scores compared
// (2 x 2K) and every product of V0's two distances (2 x K):  6K x 2^-150 = 3K x 2^-149 <= 9 x 2^-149 at K = 3.  The
// fp32 evaluation below loses at most 2^-150 more per product with a subnormal result (two of them).  The floor is
// 2^-144 = 32 x 2^-149, over three times the sum of both.  The kernel's sum fl(a + tau) rounds relative to |a| only
// (exact while a + tau is subnormal), which the relative part's er term covers as in tau_consts.  At unit scale the floor
// is 1e-38 of tau.  tests/test_tau_model.py holds the kernel's fp32 threshold against a + tau(a) + the absolute term
// in extended precision, from subnormal norms up to 1e30.
constexpr float kK1fTauFloor = 0x1p-144f;

__host__ __device__ inline float k1f_tau(float a, float x2, float y2)
{
#pragma clang fp contract(off)
    const float d = a + x2;
    return 3.8185e-6f * (x2 + y2) + 1.9074e-6f * (d > 0.0f ? d : 0.0f) + kK1fTauFloor;   // 2^-18 x 1.001, 2^-19
}

// K1f's threshold of a query whose best chunk minimum is a (xn, y2: its FMA-chain norm, the workgroup's largest ref norm)
__host__ __device__ inline float k1f_threshold(float a, float xn, float y2)
{
#pragma clang fp contract(off)
    return a + k1f_tau(a, xn * 1.00001f, y2 * 1.00001f);
}

// |value| at or above this (or NaN / INF) voids the filters' error analysis (squares overflow): the bound of K5's error
// model.  K2 keeps the largest |value| as fp32 bits (DevScalars), so the same number in both forms.
constexpr float kHuge = 1e17f;
constexpr unsigned kHugeBits = 0x5BB1A2BCu;
static_assert(__builtin_bit_cast(unsigned, kHuge) == kHugeBits, "kHugeBits is kHuge's bit pattern");
// fp16 points: K2 narrows the refs' scaled value -2 v back to binary16, finite only for |v| <= 32752 (the largest
// binary16 value whose double does not round to INF: 65504 / 2).  A larger ref value (32768 .. 65504, INF, NaN) voids the
// filter as kHuge does for the other types.  Queries are not scaled: only their NaN / INF matter.
constexpr float kF16RefMax = 32752.0f;
constexpr unsigned kF16RefMaxBits = 0x46FFE000u;
static_assert(__builtin_bit_cast(unsigned, kF16RefMax) == kF16RefMaxBits, "kF16RefMaxBits is kF16RefMax's bit pattern");
// K2's max-|ref value| word voids the filter (host latch and K5's device-side twin agree on this)
__host__ __device__ inline bool refs_void(unsigned r_maxabs_bits, bool f16)
{
    return f16 ? r_maxabs_bits > kF16RefMaxBits : r_maxabs_bits >= kHugeBits;
}

// device-side scalars shared between kernels of one index
struct DevScalars {
    unsigned r_maxabs_bits;  // max |r| bits (NaN/INF/huge detection)
    unsigned ymax2_bits;     // max centred squared norm over refs
    // the five per-search words are adjacent: one 20-byte memset resets them
    unsigned q_maxabs_bits;  // max |q| bits
    int amb_count;           // number of ambiguous queries (sent to the exact scan)
    int multi_count;         // number of queries K5 decided among MORE THAN ONE candidate within tau
    int i8_odd_count;        // int8 pre-pass: real queries whose bound B8_i exceeds 1.5 B_i (K2 on the queries)
    int i8_ran;              // int8 pre-pass: 1 when this search's filter was the pre-pass kernel (nns_index_filter_pre)
    // the int8 pre-pass of a 128-deep lazy index (K2 on the refs; fp32 bits, uint-ordered like the norms):
    unsigned i8_cmax_bits;   // largest centred |ref coordinate|, rounded up: the shared scale is s = cmax / 127
    unsigned i8_r8max2_bits; // max |r8|^2 over the refs, r8 = clamp(rint(y' / s), +-127)
    unsigned i8_eymax2_bits; // max |e_y|^2 over the refs, e_y = y' / s - r8
};

// What K2 adds for the int8 pre-pass (image_kernel<128, BF, I8>).  Refs (I8 = 1): img8 = -r8 in image_i8_kernel's lane
// map at depth 128 (1 KiB fragment 2 t + ks: point tile t, k-step ks of 64 dims; 4 KiB per 32-ref block), seeds[j] =
// floor(|y'_j|^2 / (2 s^2)) (padding refs: kI8PrePadSeed), and the two maxima above.  Queries (I8 = 2): img8 = q8 in the
// same map, bound[i] = B8_i (i8pre_bound).
struct I8PreArgs {
    uint4 *img8;
    int *seeds;
    float *bound;
    DevScalars *scal;
};
// The selection rule of the pre-pass, evaluated on the device by both filter kernels of a search (the one it does not
// name returns at once): the scale is valid — cmax finite, not huge, and not so small that 1 / (2 s^2) leaves fp32 — and,
// unless forced, at most m / 64 queries have a bound above 1.5 B (the factor and the share are conditions, not
// measurements: they cap the pre-pass's flags near lazy16's for all but a sliver of the queries).
__host__ __device__ inline bool i8pre_scale_valid(unsigned cmax_bits)
{
    const float cmax = __builtin_bit_cast(float, cmax_bits);
    return cmax >= 1e-15f && cmax < kHuge;   // (NaN: false)
}
__host__ __device__ inline bool i8pre_selected(unsigned cmax_bits, int odd_count, int m, bool force)
{
    return i8pre_scale_valid(cmax_bits) && (force || (long long)odd_count * 64 <= (long long)m);
}
// Seed of a padding ref and start value of the accumulators: above every integer threshold (<= kI8PreThrMax), and adding
// a dot product of two int8 rows (|q8.r8| <= 128 * 127^2 < 2^21) cannot overflow it.
constexpr int kI8PrePadSeed = 0x3FFFFFFF;
constexpr int kI8PreThrMax = 1 << 29;

// B8 of the int8 pre-pass: how far 2 s^2 (N_j - q8_i.r8_j) can lie ABOVE the three-product score of the pair, in score
// units.  With x' = s (q8 + e_x), y' = s (r8 + e_y):  |y'|^2 - 2 x'.y' = 2 s^2 (|y'|^2 / (2 s^2) - q8.r8) - 2 s^2 (q8.e_y +
// e_x.r8 + e_x.e_y), and Cauchy-Schwarz on the three cross terms with the refs' maxima gives
//   2 s^2 (N_j - q8.r8) <= score + 2 s^2 (|e_x| R8 + |q8| EY + |e_x| EY)        (N_j <= |y'|^2 / (2 s^2): the floor helps).
// ex2 = |e_x|^2 and q82 = |q8|^2 are the query's ACTUAL sums (a clipped coordinate is in e_x), r8max2 / eymax2 the refs'.
// c0 (tau_consts mode 3, >= 2 e3) covers the three-product score against the exact one; the factor covers the fp32
// evaluation of e_x and of the sums; two integer units (2 * 2 s^2) cover the kernel's rounding of the threshold.
__host__ __device__ inline float i8pre_bound(float s, float ex2, float q82, float r8max2, float eymax2, float c0)
{
    const double s2 = 2.0 * (double)s * (double)s;
    const double ex = sqrt((double)ex2), q8 = sqrt((double)q82), r8 = sqrt((double)r8max2), ey = sqrt((double)eymax2);
    const double b = s2 * (ex * r8 + q8 * ey + ex * ey) * (1.0 + 0x1p-10) + (double)c0 + 2.0 * s2;
    return (float)(b * (1.0 + 1e-6));
}

// ---- launchers (each .hip file owns its kernels) --------------------------------
// exact_kernels.hip
int launch_keys_fill(nns_key *keys, int m, nns_key value, hipStream_t st);
int launch_keys_min(nns_key *inout, const nns_key *other, int m, hipStream_t st);
int launch_keys_unpack(const nns_key *keys, int m, int *idx, float *dist, hipStream_t st);
int launch_fill_uniform(float *dev, size_t count, uint64_t seed, uint64_t offset, hipStream_t st);
// exact search of all m queries (K1: the nearest ref per query); the kernel codes are nns_plan_exact's
enum { EXACT_K1A = 0, EXACT_K1F = 1, EXACT_K1B = 2, EXACT_K1C = 3 };
struct ExactPlan {
    int kernel;         // EXACT_K1A (lane = query), K1F (its filter + re-rank form), K1B (lane = ref), K1C (few queries)
    int qtiles;         // query tiles (K1a / K1f: grid.x; K1b: query groups, grid.y; K1c: 1)
    int splits;         // ref ranges (K1a / K1f: grid.y; K1c: its workgroups; K1b: 0, its refs are strided over ref_wgs)
    int per;            // refs per range (the last may hold fewer)
    int waves;          // waves per workgroup
    int qt;             // queries per workgroup (K1b: the query-tile width QT)
    int ref_wgs;        // K1b: workgroups over the refs (grid.x)
    size_t ws_keys;     // merge workspace, in keys (0: none is used)
    int ws_counters;    // arrival counters that a fresh workspace has zeroed before the launch (0: nothing to arm)
};
// the plan of a search; have_ws: the merge workspace can be had (K1a falls back to one ref range per query tile
// without it, K1c to K1b); refs_aligned: the refs are 16-byte aligned (K1c's condition for k >= 4)
int exact_plan(int k, int m, int n, bool bf16, bool refs_aligned, bool have_ws, ExactPlan *p);
// ws: p.ws_keys keys for the in-kernel cross-workgroup merge; ws_fresh: it was (re)allocated or re-laid out since
// the last launch (it is then armed once; it re-arms itself).  idx_out / dist_out (optional): also write the unpacked
// indices / distances (K1a, K1f, K1c: same launch).
int launch_exact_search(const ExactPlan &p, int k, int m, int n, const void *q, const void *r, int dtype,
                        int64_t index_base, nns_key *keys, nns_key *ws, bool ws_fresh, int *idx_out, float *dist_out,
                        hipStream_t st);
// exact scan of the queries listed in qlist[0 .. *qcount) (device memory); keys
// of listed queries must hold NNS_KEY_NONE on entry (atomic-min merge).
int launch_exact_listed(int k, int n, const void *q, const void *r, int dtype, const int *qlist, const int *qcount,
                        int max_listed, int64_t index_base, nns_key *keys, hipStream_t st);

// prep_kernels.hip (K2)
int prep_workspace_bytes(int kt, size_t *bytes);
// cmax_bits (optional; the int8 pre-pass): also reduce the per-dimension minimum and maximum and leave the largest
// centred |coordinate|, rounded up, in that word (uint-ordered max: zero it first)
int launch_prep_mean(int k, int kt, int n, const float *r, double *partial_ws,
                     float *mean, unsigned *maxabs_bits, hipStream_t st, unsigned *cmax_bits = nullptr);
// K2 on one point set of an index whose geometry is g: the tile image, the norms and the scalar words of that side.
// Refs: values scaled by -2 (the int8 image holds the values themselves: -2 v does not fit, the filter applies it), padding
// refs' norm +INF, the largest norm into scal->ymax2_bits and (16-bit points; fp32 points: launch_prep_mean has written it)
// the largest |value| into scal->r_maxabs_bits; the fp32 image of a lazy-layout index in the lazy layout.  Queries: scale 1,
// padding norm 0, the largest |value| into scal->q_maxabs_bits.  8-bit points have no max-|value| word: none voids the filter.
enum PrepSide { PREP_REFS, PREP_QUERIES };
struct PrepPoints {
    int k, npts;          // dimensions and points of the set (padded to g.n_pad / g.m_pad)
    const void *pts;      // [npts][k] of g.dtype
    const float *mean;    // fp32 points: the refs' mean (launch_prep_mean)
    void *img;            // the tile image; i8pre: the int8 pre-pass's operands behind it (i8pre_layout) are written too
    float *norms;
    DevScalars *scal;
    bool i8pre;
};
int launch_prep_points(const FilterGeom &g, PrepSide side, const PrepPoints &a, hipStream_t st);
// dimension-major [k][n] -> point-major [n][k] (the inverse of the reference's mat_inv_kernel,
// core.cu:293-306); esz = 4 (fp32) or 2 (bf16 bits)
int launch_soa_to_aos(int k, int n, const void *src, void *dst, int esz, hipStream_t st);

// filter_mfma.hip (K3 fp32 / K4 bf16)
// the int8 pre-pass's operands beside the lazy image (K2, I8PreArgs): given to launch_filter, a lazy search at kt = 128
// runs filter_i8pre_kernel instead of filter_lazy16_kernel
struct FilterPreArgs {
    const char *rimg8;    // [n_pad / 32][4 KiB] + ring over-read
    const int *rseed;     // [n_pad] + ring over-read
    const float4 *q8;     // [m_pad / 16][2][64 lanes]
    const float *qb8;     // [m_pad]
    int m;                // real queries of the search
    int force;            // NNS_FILTER_I8PRE_FORCE: run the pre-pass whatever the count says
};
// What a filter plan is asked for.  form: the type's own (point_type(dtype).filter_form), or operand_form's answer for
// fp32 points; the plan's form is what is granted (SPLIT becomes F32 at a depth split_depth does not name); k beyond the
// form's deepest tile: unsupported.  per_ref: NNS_RECORDS_PER_REF; split_eager (NNS_FILTER_SPLIT_EAGER): the eager split
// kernels and image layout at every depth.  uint8 points: int8's plan field for field; only g->dtype differs
struct FilterRequest {
    int k, m, n, dtype, form;
    bool per_ref, split_eager;
};
int filter_plan(const FilterRequest &rq, FilterGeom *g);
// the tau mode of the search that geometry g runs (launch_filter and K5 agree on it)
inline int filter_tau_mode(const FilterGeom &g) { return kFilterForms[g.form].tau_mode; }
// rimg of a lazy-layout index (g.lazy_img): hi region, then the lo region at + n_pad * kt * 2 bytes
int launch_filter(const FilterGeom &g, const void *qimg, const void *rimg, const float *rnorm,
                  const float *qnorm, const DevScalars *scal, CandEntry *lists, int *counts,
                  hipStream_t st, const FilterPreArgs *pre = nullptr);
int launch_mfma_i8pre_selftest(const int8_t *q, const int8_t *r, const int *seeds, int *out, hipStream_t st);
int launch_mfma_lazy16_selftest(const float *q, const float *r, const float *c0, float *out, float *out_hh, hipStream_t st);
int filter_lazy_tile();   // MFMA tile (16 or 32) of the lazy split kernel this build launches (NNS_F_LAZY_T16)
int launch_mfma_selftest(int kt, int mode, const float *a, const float *b, const float *c0, float *out,
                         hipStream_t st);
int launch_lane_share_selftest(int t16, const float *in, float *out, hipStream_t st);

// finalize.hip (K5)
int launch_finalize(const FilterGeom &g, int k, int m, int n, const void *q, const void *r,
                    const CandEntry *lists, const int *counts, const float *qnorm,
                    DevScalars *scal, int64_t index_base, nns_key *keys, int *amb_list,
                    int *multi_list, hipStream_t st);

// topk_kernels.hip (K6: the kn nearest refs per query, exact)
struct TopkPlan {
    int qt;           // queries per workgroup
    int qgroups;      // grid.x
    int splits;       // grid.y: contiguous ref ranges, every one non-empty
    int per;          // refs per split (the last may hold fewer)
    int lds;          // LDS bytes per workgroup
    size_t ws_keys;   // split workspace [splits][m][kn] (0 with one split)
};
int topk_plan(int k, int m, int n, int kn, TopkPlan *p);
// keys[m][kn]; ws: p.ws_keys keys (unused with one split)
// bstride > 1 (K6m's sample): the scan reads every bstride-th 32-ref block of r, n counts the sampled refs
int launch_topk_search(const TopkPlan &p, int k, int m, int n, int kn, const void *q, const void *r, int dtype,
                       int64_t base, nns_key *keys, nns_key *ws, hipStream_t st, int bstride = 1);
// rows [0, rows) of ws[splits][m][kn] (m: the row stride of a split) merged into keys[rows][kn]
int launch_topk_merge_splits(const nns_key *ws, int m, int rows, int kn, int splits, nns_key *keys, hipStream_t st);
int launch_topk_merge(nns_key *inout, const nns_key *other, int m, int kn, hipStream_t st);
int launch_topk_unpack(const nns_key *keys, int m, int kn, int *idx, float *dist, hipStream_t st);

// range_kernels.hip (K7: every ref within a squared radius, CSR output)
struct RangePlan {
    int qt;           // queries per workgroup
    int qgroups;      // grid.x
    int chunks;       // grid.y: contiguous ref ranges, every one non-empty
    int per;          // refs per chunk (the last may hold fewer)
    int lds;          // LDS bytes per workgroup
    int tiles;        // tiles of the exclusive scan over the m query counts
    size_t ws_bytes;  // workspace: per-(query, chunk) counts [m][chunks] (several chunks) + tile sums (several tiles)
};
int range_plan(int k, int m, int n, RangePlan *p);
// count pass: lims[m + 1] (int64) and, with several chunks, the per-(query, chunk) start offsets in ws
int launch_range_count(const RangePlan &p, int k, int m, int n, const void *q, const void *r, int dtype, float radius2,
                       int64_t *lims, void *ws, hipStream_t st);
// fill pass: idx[lims[m]] (global indices), dist (optional) from the lims and ws of the count pass
int launch_range_fill(const RangePlan &p, int k, int m, int n, const void *q, const void *r, int dtype, float radius2,
                      int64_t base, const int64_t *lims, const void *ws, int *idx, float *dist, hipStream_t st);

// the lims scans of the count pass alone (offs: [m][chunks] counts -> offsets and lims[i + 1]; one chunk: lims[1 .. m]
// already hold the counts), shared with K7m; tiles = range_scan_tiles(m), sums: tiles int64 (several tiles)
int range_scan_tiles(int m);
int launch_range_lims(int m, int chunks, int tiles, int *offs, int64_t *sums, int64_t *lims, hipStream_t st);

// range_mfma.hip (K7m: the MFMA flag pass + V0 evaluation of the flagged 32-ref blocks)
struct RangeMfmaPlan {
    int kt, spb, qb;      // tile depth; 1 KiB fragment steps per 32-ref block; 32-query blocks per wave
    int qw;               // queries per workgroup of the flag pass
    int n_pad, total_slots, blocks, wpq;   // K2's padding; ring slots; 32-ref blocks and flag words per query
    int lazy_img;         // the ref image is in the lazy layout
    int dtype;            // DT_BF16: K2's order-1 image, range_flag16_kernel, TAU_BF16; DT_U8: the biased int8 image,
                          // range_flag_u8_kernel, the exact threshold; DT_F32: fp32 points
    int batch, batches;   // queries per flag-bitmap batch (whole workgroups), batches
    size_t flag_bytes;    // the bitmap of one batch
    int gx, gy, slots_per_split, lds;      // flag pass: grid of a full batch, slots per ref-range split, LDS bytes
    int echunks, eper;    // evaluation: chunks per query, flag words per chunk
    int tiles;            // tiles of the lims scan
    size_t offs_bytes, ws_bytes;   // K7's workspace layout: [m][echunks] counts (several chunks), then the tile sums
};
// dtype: DT_F32, DT_BF16 or DT_U8 (planned through filter_plan's int8 geometry: kt = 256, 8 fragments per block)
int range_mfma_plan(int k, int m, int n, bool split_eager, RangeMfmaPlan *p, int dtype = DT_F32);
// radius2v (optional, K6m): the batch's per-query squared radii, used instead of radius2; a query whose entry is not
// finite gets its flag row filled like a void query's; filled (optional): += the rows filled
int launch_range_flags(const RangeMfmaPlan &p, int k, int i0, int rows, const void *q, const void *qimg, const float *qnorm,
                       const void *rimg, const float *rnorm, const DevScalars *scal, float radius2, void *flags,
                       hipStream_t st, const float *radius2v = nullptr, unsigned long long *filled = nullptr);
int launch_range_eval(const RangeMfmaPlan &p, bool fill, int k, int i0, int rows, int n, const void *q, const void *r,
                      const void *flags, float radius2, int64_t base, int64_t *lims, void *ws, int *idx, float *dist,
                      unsigned long long *stat, hipStream_t st);


// topk_mfma.hip (K6m: a bound from K6's scan of a block sample, K7m's flag pass at that bound, selection among the
// flagged blocks)
struct TopkMfmaPlan {
    int stride;           // every stride-th 32-ref block is sampled (0: fewer blocks than the sample rule asks for)
    int sample_blocks;    // blocks the bound scan reads (all of them with stride <= 1)
    int sample_refs;      // refs in them (the last sampled block may be the refs' partial last block)
    int filtered;         // 1: K6m runs; 0: K6 (stride < 2, m below the filter's query floor, no flag-pass plan)
    int lds;              // LDS bytes of a selection workgroup
    size_t ws_keys;       // the index's top-K workspace: the sample scan's splits, the selection's chunks [echunks][m][kn]
    TopkPlan sp;          // filtered: K6's plan over the sample
    RangeMfmaPlan rp;     // filtered: the flag pass (its evaluation chunks are the selection's)
};
constexpr int kTopkMfmaMinQueries = 64;   // the filters' query floor
int topk_mfma_plan(int k, int m, int n, int kn, bool split_eager, TopkMfmaPlan *p, int dtype = DT_F32);
// bound[i] = the distance of keys[i][kn - 1], +INF for NNS_KEY_NONE
int launch_topk_bound(const nns_key *keys, int m, int kn, float *bound, hipStream_t st);
// the selection of one query batch: rows [i0, i0 + rows) of out[chunks][m][kn] (one chunk: the caller's keys); stat: +=
// the flagged blocks that hold a ref
int launch_topk_select(const TopkMfmaPlan &p, int k, int i0, int rows, int m, int n, int kn, const void *q, const void *r,
                       const void *flags, const float *bound, int64_t base, nns_key *out, unsigned long long *stat,
                       hipStream_t st);

}  // namespace nns
