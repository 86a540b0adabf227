"""Host-side mirror of the reference's entry point over the C ABI (include/nns.h).

The reference's operator interface for this path is a single C++ function,
``vN::cudaCall(k, m, n, s_points, r_points, &results)`` (reference
core.cu:23-29, dispatched through the function pointer of main.cu:7 and called at
main.cu:74).  ``cudaCall`` below has the same argument order and meaning and the
same result (a fresh int32 array of m global reference indices); the C++ twin is
``mi355x::cudaCall`` in csrc/nns_cudacall.hpp.  Everything else here is the
split (device-resident) API used by the tests and bench.py.

This module is plumbing: ctypes bindings to libnns_mi355x.so (hand-written HIP for
gfx950).  There is NO CPU fallback: if the library is missing the import raises,
and every entry point raises ``NNSError`` when the library reports a failure
(no device, bad arguments, HIP error) — the reference's CHECK macro prints and
exits (utils.h:16-26); a Python host gets an exception instead.
"""
from __future__ import annotations

import ctypes
import os
from typing import Callable as _Callable, NamedTuple as _NamedTuple, Optional, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NNS_LIB_PATH") or os.path.join(_HERE, "libnns_mi355x.so")   # override: A/B of builds

NNS_OK = 0
NNS_PATH_AUTO, NNS_PATH_EXACT, NNS_PATH_MFMA, NNS_PROFILE, NNS_MULTI_VIRTUAL, NNS_REFS_SOA = 0, 1, 2, 16, 32, 64
NNS_FILTER_BF16 = 128
NNS_MULTI_FORCE_COLLECTIVE = 256
NNS_KEY_NONE = 0x7F80000000000000

NNS_RECORDS_PER_REF = 512
NNS_FILTER_F32 = 1024   # fp32 points: fp32 filter operands instead of the default split-bf16 ones
NNS_FILTER_SPLIT_EAGER = 2048   # split-bf16 operands: the eager schedule (three products per tile) at every depth
# range search through the MFMA flag pass (K7m) / top-K through the bound / flag / select path (K6m): fp32 points on
# split-bf16 operands, 8 <= k <= 256; bf16 points on exact operands and uint8 points on the int8 MFMA, 32 <= k <= 256
NNS_RANGE_MFMA = 4096
NNS_TOPK_MFMA = 8192
# the int8 pre-pass of the 128-deep lazy filter: off / force ("auto": neither; the device decides per search)
NNS_FILTER_I8PRE_OFF = 16384
NNS_FILTER_I8PRE_FORCE = 32768
_I8PRE = {"auto": 0, "off": NNS_FILTER_I8PRE_OFF, "force": NNS_FILTER_I8PRE_FORCE}
# "mfma_perref": the MFMA filter with per-score candidate records forced (the long-stream form) at any size
_PATHS = {"auto": NNS_PATH_AUTO, "exact": NNS_PATH_EXACT, "mfma": NNS_PATH_MFMA,
          "mfma_perref": NNS_PATH_MFMA | NNS_RECORDS_PER_REF}

# every symbol include/nns.h declares (tests check the library exports them all)
ABI_SYMBOLS = (
    "nns_search_f32", "nns_search_f32_ex", "nns_index_create", "nns_index_destroy",
    "nns_index_refresh", "nns_index_search", "nns_index_stats", "nns_keys_min",
    "nns_keys_unpack", "nns_fill_uniform", "nns_device_count", "nns_strerror",
    "nns_last_error", "nns_version", "nns_selftest_mfma",
    "nns_index_create_bf16", "nns_index_search_bf16", "nns_search_bf16_ex", "nns_search_f32_multi",
    "nns_trim", "nns_warmup", "nns_shutdown", "nns_search_bf16_multi",
    "nns_index_near_ties", "nns_tau_consts", "nns_index_search_indices", "nns_selftest_lane_share", "nns_plan_filter", "nns_plan_exact",
    "nns_comm_unique_id", "nns_comm_create", "nns_comm_size", "nns_comm_allreduce_min", "nns_comm_destroy",
    "nns_multi_last_exchange_ranks", "nns_index_filter_form", "nns_selftest_mfma_lazy", "nns_split_lazy_bound",
    "nns_index_search_topk", "nns_keys_topk_merge", "nns_keys_topk_unpack", "nns_search_f32_topk",
    "nns_search_bf16_topk", "nns_plan_topk",
    "nns_index_range_count", "nns_index_range_fill", "nns_search_f32_range", "nns_search_bf16_range", "nns_plan_range",
    "nns_index_range_info", "nns_plan_range_mfma", "nns_range_threshold",
    "nns_index_topk_info", "nns_plan_topk_mfma",
    "nns_filter_lazy_tile", "nns_selftest_mfma_lazy16",
    "nns_plan_range_mfma_bf16", "nns_plan_topk_mfma_bf16", "nns_range_threshold_bf16",
    "nns_index_create_f16", "nns_index_search_f16", "nns_search_f16_ex", "nns_search_f16_topk", "nns_search_f16_range",
    "nns_index_create_i8", "nns_index_search_i8", "nns_search_i8_ex", "nns_search_i8_topk", "nns_search_i8_range",
    "nns_index_create_b1", "nns_index_search_b1", "nns_search_b1_ex", "nns_search_b1_topk", "nns_search_b1_range",
    "nns_index_filter_pre", "nns_i8pre_bound", "nns_selftest_mfma_i8pre",
    "nns_index_create_u8", "nns_index_search_u8", "nns_search_u8_ex", "nns_search_u8_topk", "nns_search_u8_range",
    "nns_plan_range_mfma_u8", "nns_plan_topk_mfma_u8", "nns_range_threshold_u8",
)
# the newest of them: a build from before they existed, loaded through NNS_LIB_PATH as an A/B arm, may lack these (they
# then fail when called); build() requires every symbol of the tree's own library
OPTIONAL_SYMBOLS = ("nns_filter_lazy_tile", "nns_selftest_mfma_lazy16",
                    "nns_plan_range_mfma_bf16", "nns_plan_topk_mfma_bf16", "nns_range_threshold_bf16",
                    "nns_index_create_f16", "nns_index_search_f16", "nns_search_f16_ex", "nns_search_f16_topk",
                    "nns_search_f16_range",
                    "nns_index_create_i8", "nns_index_search_i8", "nns_search_i8_ex", "nns_search_i8_topk",
                    "nns_search_i8_range",
                    "nns_index_create_b1", "nns_index_search_b1", "nns_search_b1_ex", "nns_search_b1_topk",
                    "nns_search_b1_range",
                    "nns_index_filter_pre", "nns_i8pre_bound", "nns_selftest_mfma_i8pre",
                    "nns_index_create_u8", "nns_index_search_u8", "nns_search_u8_ex", "nns_search_u8_topk",
                    "nns_search_u8_range", "nns_plan_range_mfma_u8", "nns_plan_topk_mfma_u8", "nns_range_threshold_u8")
NNS_TOPK_MAX = 256
NNS_COMM_ID_BYTES = 128


class NNSError(RuntimeError):
    """A C-ABI call returned a non-zero status."""

    def __init__(self, status: int, where: str, detail: str):
        super().__init__(f"{where}: status {status} ({detail})")
        self.status = status


class nns_stats(ctypes.Structure):
    _fields_ = [
        ("path", ctypes.c_int), ("k_tile", ctypes.c_int), ("splits", ctypes.c_int),
        ("ambiguous", ctypes.c_int), ("nonfinite", ctypes.c_int),
        ("prep_refs_ms", ctypes.c_float), ("prep_queries_ms", ctypes.c_float),
        ("filter_ms", ctypes.c_float), ("finalize_ms", ctypes.c_float),
        ("rerank_ms", ctypes.c_float), ("exact_ms", ctypes.c_float),
        ("total_ms", ctypes.c_float), ("multi_candidate", ctypes.c_int),
    ]

    def asdict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


# ---- host arrays as the library reads them, per point type ----------------------------------------------------------
def _as_f32(a, what: str) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2:
        raise ValueError(f"{what} must be [points][k]")
    return a


def _as_bf16_bits(a) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.uint16)
    if a.ndim != 2:
        raise ValueError("bf16 point sets must be 2-D arrays of bit patterns")
    return a


def to_f16_bits(a) -> np.ndarray:
    """A numpy float16 array, or uint16 bit patterns, as contiguous 2-D uint16 binary16 bit patterns (no conversion of
    values: other dtypes are refused, so that nothing is rounded silently)."""
    a = np.asarray(a)
    if a.dtype == np.float16:
        a = np.ascontiguousarray(a).view(np.uint16)
    elif a.dtype != np.uint16:
        raise ValueError("fp16 point sets must be numpy float16 arrays or uint16 bit patterns")
    a = np.ascontiguousarray(a)
    if a.ndim != 2:
        raise ValueError("fp16 point sets must be 2-D arrays")
    return a


def to_i8(a) -> np.ndarray:
    """A numpy int8 array as a contiguous 2-D int8 array (other dtypes are refused: nothing is quantised silently)."""
    a = np.asarray(a)
    if a.dtype != np.int8:
        raise ValueError("int8 point sets must be numpy int8 arrays")
    a = np.ascontiguousarray(a)
    if a.ndim != 2:
        raise ValueError("int8 point sets must be 2-D arrays")
    return a


def to_u8(a) -> np.ndarray:
    """A numpy uint8 array as a contiguous 2-D uint8 array of point values 0 .. 255 (other dtypes are refused: nothing is
    quantised silently)."""
    a = np.asarray(a)
    if a.dtype != np.uint8:
        raise ValueError("uint8 point sets must be numpy uint8 arrays")
    a = np.ascontiguousarray(a)
    if a.ndim != 2:
        raise ValueError("uint8 point sets must be 2-D arrays")
    return a


def to_b1(a) -> np.ndarray:
    """Packed binary points, numpy uint8 [.][kb] with kb % 4 == 0 or uint32 [.][kw], as a contiguous uint8 [.][4 * kw]
    array (anything else, a buffer that is not 4-byte aligned included, is refused)."""
    a = np.asarray(a)
    if a.ndim != 2 or a.dtype not in (np.uint8, np.uint32):
        raise ValueError("binary point sets must be 2-D numpy uint8 or uint32 arrays of packed bits (see pack_bits)")
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.uint8)
    if a.shape[1] % 4 != 0:
        raise ValueError("binary point sets hold whole 32-bit words: the byte count per point must be a multiple of 4")
    if a.ctypes.data % 4 != 0:   # (a view into a byte buffer: the library reads words)
        raise ValueError("binary point sets must be 4-byte aligned")
    return a


class _PointType(_NamedTuple):
    """One point type: what differs between the per-dtype entry points and their wrappers here."""
    code: int            # the C ABI's dtype code (nns_plan_*'s bf16_points; the bf16= arguments here take it)
    infix: str           # nns_search_<infix>_ex, nns_index_create_<infix>
    convert: _Callable   # host array -> the contiguous 2-D array the library reads
    k_mult: int          # k per array column (packed bits: 8 per byte)
    refs_soa: bool       # dimension-major refs are offered
    mfma_flags: bool     # range_mfma / topk_mfma are offered

    def search_name(self, what: str) -> str:
        return f"nns_search_{self.infix}_{what}"

    def index_name(self, what: str) -> str:
        return f"nns_index_{what}" + ("" if self.code == 0 else "_" + self.infix)   # (the fp32 ones carry no infix)


_POINT_TYPES = {pt.code: pt for pt in (
    _PointType(0, "f32", lambda a: _as_f32(a, "points"), 1, True, True),
    _PointType(1, "bf16", _as_bf16_bits, 1, True, True),
    _PointType(2, "f16", to_f16_bits, 1, True, False),
    _PointType(3, "i8", to_i8, 1, False, False),
    _PointType(4, "b1", to_b1, 8, False, False),
    _PointType(5, "u8", to_u8, 1, False, True))}


def _load() -> ctypes.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C nns-cuda_amd/csrc`). The HIP extension is the product; there is no CPU fallback.")
    # If torch is (going to be) in the process, let it bring the HIP runtime first so
    # that one libamdhip64.so.7 serves both (same SONAME in torch/lib and /opt/rocm).
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is optional for the host-buffer API
        pass
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    c_int, c_vp, c_sz, c_u64, c_i64, c_u = (ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                             ctypes.c_uint64, ctypes.c_int64, ctypes.c_uint)
    lib.nns_search_f32.argtypes = [c_int, c_int, c_int, c_vp, c_vp, ctypes.POINTER(ctypes.POINTER(c_int))]
    # the five per-dtype families: one signature each, whatever the element type
    per_dtype = {}
    for pt in _POINT_TYPES.values():
        per_dtype[pt.index_name("create")] = [ctypes.POINTER(c_vp), c_int, c_int, c_int, c_vp, c_i64, c_u, c_vp]
        per_dtype[pt.index_name("search")] = [c_vp, c_int, c_vp, c_vp, c_vp]
        per_dtype[pt.search_name("ex")] = [c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_int, c_u, c_int]
        per_dtype[pt.search_name("topk")] = [c_int, c_int, c_int, c_vp, c_vp, c_int, c_vp, c_vp, c_int, c_u, c_int]
        per_dtype[pt.search_name("range")] = [c_int, c_int, c_int, c_vp, c_vp, ctypes.c_float, c_vp,
                                              ctypes.POINTER(ctypes.POINTER(c_int)),
                                              ctypes.POINTER(ctypes.POINTER(ctypes.c_float)), c_u, c_int]
    for name, argtypes in per_dtype.items():
        if name not in OPTIONAL_SYMBOLS:
            getattr(lib, name).argtypes = argtypes
    lib.nns_search_f32_multi.argtypes = [c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_int, c_u]
    lib.nns_search_bf16_multi.argtypes = lib.nns_search_f32_multi.argtypes
    lib.nns_comm_unique_id.argtypes = [c_vp, c_sz]
    lib.nns_comm_create.argtypes = [ctypes.POINTER(c_vp), c_vp, c_sz, c_int, c_int, c_int]
    lib.nns_comm_size.argtypes = [c_vp]
    lib.nns_comm_allreduce_min.argtypes = [c_vp, c_vp, c_int, c_vp]
    lib.nns_comm_destroy.argtypes = [c_vp]
    lib.nns_shutdown.argtypes = []
    lib.nns_multi_last_exchange_ranks.argtypes = []
    lib.nns_index_destroy.argtypes = [c_vp]
    lib.nns_index_refresh.argtypes = [c_vp, c_vp]
    lib.nns_index_stats.argtypes = [c_vp, ctypes.POINTER(nns_stats)]
    lib.nns_index_search_indices.argtypes = [c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_vp]
    lib.nns_index_near_ties.argtypes = [c_vp, c_vp, c_int, ctypes.POINTER(c_int)]
    lib.nns_tau_consts.argtypes = [c_int, ctypes.c_float, ctypes.c_float, c_int, c_vp]
    lib.nns_selftest_lane_share.argtypes = [c_int, c_vp, c_vp]
    lib.nns_plan_filter.argtypes = [c_int, c_int, c_int, c_int, c_u, c_vp, c_int]
    lib.nns_index_filter_form.argtypes = [c_vp, ctypes.POINTER(c_int)]
    lib.nns_plan_exact.argtypes = [c_int, c_int, c_int, c_int, c_int, c_vp, c_int]
    lib.nns_keys_min.argtypes = [c_vp, c_vp, c_int, c_vp]
    lib.nns_keys_unpack.argtypes = [c_vp, c_int, c_vp, c_vp, c_vp]
    lib.nns_fill_uniform.argtypes = [c_vp, c_sz, c_u64, c_u64, c_vp]
    lib.nns_selftest_mfma.argtypes = [c_int, c_int, c_vp, c_vp, c_vp, c_vp]
    lib.nns_selftest_mfma_lazy.argtypes = [c_int, c_vp, c_vp, c_vp, c_vp, c_vp]
    lib.nns_split_lazy_bound.argtypes = [c_int, ctypes.c_float, ctypes.c_float, c_vp]
    lib.nns_index_search_topk.argtypes = [c_vp, c_int, c_vp, c_int, c_vp, c_vp]
    lib.nns_keys_topk_merge.argtypes = [c_vp, c_vp, c_int, c_int, c_vp]
    lib.nns_keys_topk_unpack.argtypes = [c_vp, c_int, c_int, c_vp, c_vp, c_vp]
    lib.nns_plan_topk.argtypes = [c_int, c_int, c_int, c_int, c_int, c_vp, c_int]
    lib.nns_index_range_count.argtypes = [c_vp, c_int, c_vp, ctypes.c_float, c_vp, c_vp]
    lib.nns_index_range_fill.argtypes = [c_vp, c_int, c_vp, ctypes.c_float, c_vp, c_vp, c_vp, c_vp]
    lib.nns_plan_range.argtypes = [c_int, c_int, c_int, c_int, c_vp, c_int]
    lib.nns_index_range_info.argtypes = [c_vp, c_vp, c_int]
    lib.nns_plan_range_mfma.argtypes = [c_int, c_int, c_int, c_u, c_vp, c_int]
    lib.nns_range_threshold.argtypes = [c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float, c_vp]
    lib.nns_index_topk_info.argtypes = [c_vp, c_vp, c_int]
    lib.nns_plan_topk_mfma.argtypes = [c_int, c_int, c_int, c_int, c_u, c_vp, c_int]
    lib.nns_device_count.argtypes = []
    lib.nns_strerror.argtypes = [c_int]
    lib.nns_strerror.restype = ctypes.c_char_p
    lib.nns_last_error.argtypes = []
    lib.nns_last_error.restype = ctypes.c_char_p
    lib.nns_version.argtypes = []
    optional = {"nns_filter_lazy_tile": [], "nns_selftest_mfma_lazy16": [c_vp, c_vp, c_vp, c_vp, c_vp],
                "nns_plan_range_mfma_bf16": lib.nns_plan_range_mfma.argtypes,
                "nns_plan_topk_mfma_bf16": lib.nns_plan_topk_mfma.argtypes,
                "nns_range_threshold_bf16": lib.nns_range_threshold.argtypes,
                "nns_index_filter_pre": [c_vp, ctypes.POINTER(c_int)],
                "nns_i8pre_bound": [ctypes.c_float] * 6 + [c_vp],
                "nns_selftest_mfma_i8pre": [c_vp, c_vp, c_vp, c_vp],
                "nns_plan_range_mfma_u8": lib.nns_plan_range_mfma.argtypes,
                "nns_plan_topk_mfma_u8": lib.nns_plan_topk_mfma.argtypes,
                "nns_range_threshold_u8": [ctypes.c_float, ctypes.c_float, c_vp]}
    optional.update({name: argtypes for name, argtypes in per_dtype.items() if name in OPTIONAL_SYMBOLS})
    assert set(optional) == set(OPTIONAL_SYMBOLS)
    absent = tuple(n for n in OPTIONAL_SYMBOLS if not hasattr(lib, n))
    for name, argtypes in optional.items():
        if name not in absent:
            getattr(lib, name).argtypes = argtypes
    for name in ABI_SYMBOLS:
        if name not in ("nns_strerror", "nns_last_error", "nns_trim") + absent:
            getattr(lib, name).restype = c_int
    lib.nns_warmup.argtypes = [c_int]
    lib.nns_trim.argtypes = []
    lib.nns_trim.restype = ctypes.c_size_t
    return lib


lib = _load()
_libc = ctypes.CDLL(None)
_libc.free.argtypes = [ctypes.c_void_p]


def _check(status: int, where: str) -> None:
    if status != NNS_OK:
        detail = lib.nns_last_error().decode() or lib.nns_strerror(status).decode()
        raise NNSError(status, where, detail)


def selftest_mfma(a: np.ndarray, b: np.ndarray, c0: np.ndarray, bf16: int = 0) -> np.ndarray:
    """out[i][j] of one 32x32 MFMA tile (diagnostic, see include/nns.h).  bf16: 0 fp32, 1 bf16 32x32x16, 2 bf16
    16x16x32, 3 the split chain of fp32 values, 5 f16 16x16x32 (the values cast to binary16), 6 i8 16x16x64 (the values
    cast to int8, i32 accumulation seeded with int(c0), returned as fp32; kt a multiple of 64)."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    c0 = np.ascontiguousarray(c0, np.float32)
    assert a.shape == b.shape and a.shape[0] == 32 and c0.shape == (32,)
    out = np.empty((32, 32), np.float32)
    _check(lib.nns_selftest_mfma(a.shape[1], int(bf16), a.ctypes.data, b.ctypes.data, c0.ctypes.data, out.ctypes.data),
           "nns_selftest_mfma")
    return out


def selftest_mfma_lazy(a: np.ndarray, b: np.ndarray, c0: np.ndarray):
    """(out, out_hh) of nns_selftest_mfma_lazy: the split chain in the lazy filter's order and its hi.hi partial."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    c0 = np.ascontiguousarray(c0, np.float32)
    assert a.shape == b.shape and a.shape[0] == 32 and c0.shape == (32,)
    out = np.empty((32, 32), np.float32)
    out_hh = np.empty((32, 32), np.float32)
    _check(lib.nns_selftest_mfma_lazy(a.shape[1], a.ctypes.data, b.ctypes.data, c0.ctypes.data, out.ctypes.data,
                                      out_hh.ctypes.data), "nns_selftest_mfma_lazy")
    return out, out_hh


def selftest_mfma_lazy16(q: np.ndarray, r: np.ndarray, c0: np.ndarray):
    """(out, out_hh) of nns_selftest_mfma_lazy16, [32 refs][64 queries] each: the lazy split chain on 16x16x32 MFMAs
    (operands gathered from images in the 32x32x16 order) and its hi.hi partial.  q [64][128], r [32][128], c0 [32]."""
    q = np.ascontiguousarray(q, np.float32)
    r = np.ascontiguousarray(r, np.float32)
    c0 = np.ascontiguousarray(c0, np.float32)
    assert q.shape == (64, 128) and r.shape == (32, 128) and c0.shape == (32,)
    out = np.empty((32, 64), np.float32)
    out_hh = np.empty((32, 64), np.float32)
    _check(lib.nns_selftest_mfma_lazy16(q.ctypes.data, r.ctypes.data, c0.ctypes.data, out.ctypes.data, out_hh.ctypes.data),
           "nns_selftest_mfma_lazy16")
    return out, out_hh


def selftest_mfma_i8pre(q: np.ndarray, r: np.ndarray, seeds: np.ndarray) -> np.ndarray:
    """nns_selftest_mfma_i8pre: [32 refs][64 queries] int32 accumulators seeds[ref] - q.r of the int8 pre-pass's chain.
    q [64][128], r [32][128] int8, seeds [32] int32."""
    q = np.ascontiguousarray(q, np.int8)
    r = np.ascontiguousarray(r, np.int8)
    seeds = np.ascontiguousarray(seeds, np.int32)
    assert q.shape == (64, 128) and r.shape == (32, 128) and seeds.shape == (32,)
    out = np.empty((32, 64), np.int32)
    _check(lib.nns_selftest_mfma_i8pre(q.ctypes.data, r.ctypes.data, seeds.ctypes.data, out.ctypes.data), "nns_selftest_mfma_i8pre")
    return out


def filter_lazy_tile() -> int:
    """nns_filter_lazy_tile: 16 or 32, the MFMA tile of the lazy split kernel this build launches."""
    return int(lib.nns_filter_lazy_tile())


def i8pre_bound(s: float, ex2: float, q82: float, r8max2: float, eymax2: float, c0: float) -> float:
    """B8 of the int8 pre-pass for one query (nns_i8pre_bound)."""
    out = np.empty(1, np.float32)
    _check(lib.nns_i8pre_bound(s, ex2, q82, r8max2, eymax2, c0, out.ctypes.data), "nns_i8pre_bound")
    return float(out[0])


def split_lazy_bound(kt: int, qnorm2: float, ymax2: float) -> float:
    """B of the lazy split filter (nns_split_lazy_bound)."""
    out = np.empty(1, np.float32)
    _check(lib.nns_split_lazy_bound(kt, qnorm2, ymax2, out.ctypes.data), "nns_split_lazy_bound")
    return float(out[0])


def plan_filter(k: int, m: int, n: int, bf16: bool = False, flags: int = 0, schedule: bool = False) -> dict:
    """nns_plan_filter: the MFMA filter's launch geometry for a shape (host only).  bf16: False / True, 2 for fp16 or 3
    for int8, 5 for uint8 points (here and in plan_topk / plan_range; those two also take 4, binary points, with k in bits).  "split": 1 when fp32 points
    take split-bf16 operands (the default; NNS_FILTER_F32 in flags: fp32 operands, 0).  schedule=True asks for the
    16th field too, "lazy": 1 when the split operands run the lazy schedule (0 with NNS_FILTER_SPLIT_EAGER)."""
    nf = 16 if schedule else 15
    out = np.zeros(nf, np.int32)
    _check(lib.nns_plan_filter(k, m, n, int(bf16), flags, out.ctypes.data, nf), "nns_plan_filter")
    names = ("kt", "bf16", "mixed", "lpq", "m_pad", "n_pad", "total_slots", "splits", "slots_per_split", "qgroups",
             "slot_pts", "queries_per_wg", "share_thr", "tile_rec", "split", "lazy")[:nf]
    return dict(zip(names, (int(v) for v in out)))


def plan_exact(k: int, m: int, n: int, refs_aligned: bool = True, have_workspace: bool = True) -> dict:
    """nns_plan_exact: the exact path's launch geometry for a shape (host only)."""
    out = np.zeros(6, np.int32)
    _check(lib.nns_plan_exact(k, m, n, int(refs_aligned), int(have_workspace), out.ctypes.data, 6), "nns_plan_exact")
    names = ("kernel", "qtiles", "splits", "per", "waves", "queries_per_wg")
    d = dict(zip(names, (int(v) for v in out)))
    d["kernel"] = ("k1a", "k1f", "k1b", "k1c")[d["kernel"]]
    return d


def plan_topk(k: int, m: int, n: int, kn: int, bf16: bool = False) -> dict:
    """nns_plan_topk: the top-K (K6) launch geometry for a shape (host only)."""
    out = np.zeros(6, np.int32)
    _check(lib.nns_plan_topk(k, m, n, kn, int(bf16), out.ctypes.data, 6), "nns_plan_topk")
    names = ("queries_per_wg", "splits", "per", "workgroups", "lds_bytes", "ws_keys")
    return dict(zip(names, (int(v) for v in out)))


def plan_range(k: int, m: int, n: int, bf16: bool = False) -> dict:
    """nns_plan_range: the range search (K7) launch geometry for a shape (host only)."""
    out = np.zeros(6, np.int32)
    _check(lib.nns_plan_range(k, m, n, int(bf16), out.ctypes.data, 6), "nns_plan_range")
    names = ("queries_per_wg", "chunks", "per", "workgroups", "lds_bytes", "ws_bytes")
    return dict(zip(names, (int(v) for v in out)))


# the flag-pass plans of the point types that have one (any other code: the bf16 plan)
_FLAG_PLAN_SUFFIX = {0: "", 1: "_bf16", 5: "_u8"}


def plan_range_mfma(k: int, m: int, n: int, flags: int = 0, *, bf16: bool = False) -> dict:
    """nns_plan_range_mfma: the launch geometry of the MFMA-filtered range search (K7m) for a shape (host only);
    flags: the index's (NNS_FILTER_SPLIT_EAGER selects the eager ref image layout).  bf16: the plan for bf16 points
    (nns_plan_range_mfma_bf16; layout 2 = the order-1 16x16x32 image); bf16=5: the plan for uint8 points
    (nns_plan_range_mfma_u8; kt = 256, layout 3 = the int8 image)."""
    out = np.zeros(10, np.int32)
    name = "nns_plan_range_mfma" + _FLAG_PLAN_SUFFIX.get(int(bf16), "_bf16")
    _check(getattr(lib, name)(k, m, n, flags, out.ctypes.data, 10), name)
    names = ("kt", "block_refs", "blocks_per_query", "batch", "batches", "flag_ws_bytes", "grid_x", "grid_y", "lds_bytes",
             "layout")
    return dict(zip(names, (int(v) for v in out)))


def plan_topk_mfma(k: int, m: int, n: int, kn: int, flags: int = 0, *, bf16: bool = False) -> dict:
    """nns_plan_topk_mfma: the plan of the MFMA-filtered top-K search (K6m) for a shape (host only): the block sample of
    the bound scan, whether the filtered path is taken, and then plan_range_mfma's fields, the selection's chunks per
    query and flag words per chunk (zeros otherwise), and the LDS bytes of a selection workgroup.  bf16: the plan for
    bf16 points (nns_plan_topk_mfma_bf16); bf16=5: for uint8 points (nns_plan_topk_mfma_u8)."""
    out = np.zeros(17, np.int32)
    name = "nns_plan_topk_mfma" + _FLAG_PLAN_SUFFIX.get(int(bf16), "_bf16")
    _check(getattr(lib, name)(k, m, n, kn, flags, out.ctypes.data, 17), name)
    names = ("sample_blocks", "stride", "sample_refs", "filtered", "kt", "block_refs", "blocks_per_query", "batch",
             "batches", "flag_ws_bytes", "grid_x", "grid_y", "lds_bytes", "layout", "chunks", "chunk_words",
             "select_lds_bytes")
    return dict(zip(names, (int(v) for v in out)))


def range_threshold(kt: int, qnorm2: float, ymax2: float, radius2: float, *, bf16: bool = False) -> float:
    """nns_range_threshold: the score threshold K7m's flag pass gives a query (host only).  bf16: the threshold of a
    bf16 query (nns_range_threshold_bf16: exact operands, uncentred norms)."""
    out = np.zeros(1, np.float32)
    if bf16:
        _check(lib.nns_range_threshold_bf16(kt, qnorm2, ymax2, radius2, out.ctypes.data), "nns_range_threshold_bf16")
    else:
        _check(lib.nns_range_threshold(kt, qnorm2, ymax2, radius2, out.ctypes.data), "nns_range_threshold")
    return float(out[0])


def range_threshold_u8(qnorm2: float, radius2: float) -> float:
    """nns_range_threshold_u8: the exact score threshold of a uint8 query of biased squared norm qnorm2 (host only)."""
    out = np.zeros(1, np.float32)
    _check(lib.nns_range_threshold_u8(qnorm2, radius2, out.ctypes.data), "nns_range_threshold_u8")
    return float(out[0])


def selftest_lane_share(values, tile16: bool) -> np.ndarray:
    """out[l] of nns_selftest_lane_share for 64 lane values."""
    v = np.ascontiguousarray(values, np.float32)
    assert v.shape == (64,)
    out = np.empty(64, np.float32)
    _check(lib.nns_selftest_lane_share(int(tile16), v.ctypes.data, out.ctypes.data), "nns_selftest_lane_share")
    return out


def tau_consts(kt: int, qnorm2: float, ymax2: float, mode: int):
    """(c0, c1, x2) of the proof margin tau(a) = c0 + c1 * max(a + x2, 0) (nns_tau_consts; mode 0 .. 4, 4: fp16 points)."""
    out = np.empty(3, np.float32)
    _check(lib.nns_tau_consts(kt, qnorm2, ymax2, mode, out.ctypes.data), "nns_tau_consts")
    return float(out[0]), float(out[1]), float(out[2])


def device_count() -> int:
    return lib.nns_device_count()


def cudaCall(k: int, m: int, n: int, s_points, r_points) -> np.ndarray:
    """Drop-in for the reference's ``vN::cudaCall(k, m, n, s_points, r_points, &results)``.

    s_points: m*k fp32 (row-major queries), r_points: n*k fp32 (row-major refs);
    returns the malloc'd int32[m] result the C ABI hands back, copied into numpy.
    """
    s = np.ascontiguousarray(s_points, dtype=np.float32).reshape(-1)
    r = np.ascontiguousarray(r_points, dtype=np.float32).reshape(-1)
    if s.size < k * m or r.size < k * n:
        raise ValueError("point arrays shorter than k*m / k*n")
    res = ctypes.POINTER(ctypes.c_int)()
    _check(lib.nns_search_f32(k, m, n, s.ctypes.data, r.ctypes.data, ctypes.byref(res)), "nns_search_f32")
    try:
        return np.ctypeslib.as_array(res, shape=(m,)).astype(np.int32, copy=True)
    finally:
        _libc.free(res)


def _search_1nn(code, query_points, reference_points, return_distances, shards, path, device, refs_soa=False, flags=0):
    """The whole-call nearest-neighbour search of point type `code` (nns_search_<infix>_ex)."""
    pt = _POINT_TYPES[code]
    assert pt.refs_soa or not refs_soa
    q = pt.convert(query_points)
    r = pt.convert(reference_points)
    if q.shape[1] != (r.shape[0] if refs_soa else r.shape[1]):
        raise ValueError("query and reference dimensionality differ")
    m, cols = q.shape
    n = r.shape[1] if refs_soa else r.shape[0]
    idx = np.empty(m, dtype=np.int32)
    dist = np.empty(m, dtype=np.float32) if return_distances else None
    name = pt.search_name("ex")
    _check(getattr(lib, name)(cols * pt.k_mult, m, n, q.ctypes.data, r.ctypes.data, idx.ctypes.data,
                              dist.ctypes.data if dist is not None else None, shards,
                              _PATHS[path] | (NNS_REFS_SOA if refs_soa else 0) | flags, device), name)
    return (idx, dist) if return_distances else idx


def search(query_points, reference_points, *, return_distances: bool = False, shards: int = 1,
           path: str = "auto", device: int = 0, refs_soa: bool = False, filter_bf16: bool = False):
    """``search(query_points, reference_points)`` — the entry point BASELINE.json names.

    Host arrays in, nearest-reference index per query out (and, optionally, V0's
    fp32 squared distance).  ``shards`` > 1 rehearses the multi-GPU ref split on one
    device (contiguous ceil(n/shards) ranges merged with the packed-key min).  ``refs_soa``:
    reference_points is dimension-major [k][n] (NNS_REFS_SOA, the reference's V4 layout)."""
    q = _as_f32(query_points, "query_points")
    r = _as_f32(reference_points, "reference_points")
    return _search_1nn(0, q, r, return_distances, shards, path, device, refs_soa, NNS_FILTER_BF16 if filter_bf16 else 0)


def search_multi(query_points, reference_points, *, num_devices: int = 0, return_distances: bool = False,
                 path: str = "auto", virtual: bool = False, refs_soa: bool = False, bf16: bool = False,
                 force_collective: bool = False):
    """The V8/V9 analogue: refs sharded over `num_devices` GPUs of this process (0 = all),
    per-GPU keys combined with one RCCL min all-reduce.  `virtual` lets a 1-GPU box rehearse
    more shards than it has GPUs (host-side key merge).  `bf16`: the arrays hold bf16 bit
    patterns (uint16); `refs_soa`: reference_points is dimension-major [k][n].  `force_collective`
    (tests): no single-GPU shortcut, so that ncclCommInitAll + the grouped all-reduce also run with one
    shard on a one-GPU box (NNS_MULTI_FORCE_COLLECTIVE)."""
    if bf16:
        q = _as_bf16_bits(query_points)
        r = _as_bf16_bits(reference_points)
    else:
        q = _as_f32(query_points, "query_points")
        r = _as_f32(reference_points, "reference_points")
    if q.shape[1] != (r.shape[0] if refs_soa else r.shape[1]):
        raise ValueError("query and reference dimensionality differ")
    m, k = q.shape
    n = r.shape[1] if refs_soa else r.shape[0]
    idx = np.empty(m, dtype=np.int32)
    dist = np.empty(m, dtype=np.float32) if return_distances else None
    flags = _PATHS[path] | (NNS_MULTI_VIRTUAL if virtual else 0) | (NNS_REFS_SOA if refs_soa else 0) \
        | (NNS_MULTI_FORCE_COLLECTIVE if force_collective else 0)
    fn = lib.nns_search_bf16_multi if bf16 else lib.nns_search_f32_multi
    _check(fn(k, m, n, q.ctypes.data, r.ctypes.data, idx.ctypes.data,
              dist.ctypes.data if dist is not None else None, num_devices, flags), "nns_search_multi")
    return (idx, dist) if return_distances else idx


def to_bf16_bits(a) -> np.ndarray:
    """fp32 array -> bf16 bit patterns (uint16), round-to-nearest-even (NaN stays NaN)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(a)
    if nan.any():
        r[nan] = ((u[nan] >> 16) | 0x0040).astype(np.uint16)
    return r


def search_bf16(query_bits, reference_bits, *, return_distances: bool = False, shards: int = 1,
                path: str = "auto", device: int = 0):
    """search() for bf16 point sets given as uint16 bit patterns [points][k] (config C5):
    V0's arithmetic on the bf16 values widened to fp32."""
    q = np.ascontiguousarray(query_bits, dtype=np.uint16)
    r = np.ascontiguousarray(reference_bits, dtype=np.uint16)
    if q.ndim != 2 or r.ndim != 2 or q.shape[1] != r.shape[1]:
        raise ValueError("bf16 point sets must be [points][k] with equal k")
    return _search_1nn(1, q, r, return_distances, shards, path, device)


def search_f16(query_points, reference_points, *, return_distances: bool = False, shards: int = 1,
               path: str = "auto", device: int = 0, refs_soa: bool = False):
    """search() for fp16 point sets (numpy float16, or uint16 binary16 bit patterns) [points][k]: V0's arithmetic on the
    values widened exactly to fp32 (nns_search_f16_ex).  refs_soa: reference_points is dimension-major [k][n]."""
    return _search_1nn(2, query_points, reference_points, return_distances, shards, path, device, refs_soa)


def search_i8(query_points, reference_points, *, return_distances: bool = False, shards: int = 1,
              path: str = "auto", device: int = 0):
    """search() for int8 point sets (numpy int8) [points][k]: V0's arithmetic on the values widened exactly to fp32
    (nns_search_i8_ex).  For k <= 256 the distances are the exact integer squared distances."""
    return _search_1nn(3, query_points, reference_points, return_distances, shards, path, device)


def search_u8(query_points, reference_points, *, return_distances: bool = False, shards: int = 1,
              path: str = "auto", device: int = 0):
    """search() for uint8 point sets (numpy uint8, values 0 .. 255) [points][k]: V0's arithmetic on the values widened
    exactly to fp32 (nns_search_u8_ex).  For k <= 256 the distances are the exact integer squared distances."""
    return _search_1nn(5, query_points, reference_points, return_distances, shards, path, device)


def pack_bits(a) -> np.ndarray:
    """A [n][k] array of bool / 0-1 values as packed binary points: uint8 [n][4 * ceil(k / 32)], bit t of a point at
    (byte[t // 8] >> (t % 8)) & 1 (= bit t % 32 of little-endian word t // 32), zero-padded to whole 32-bit words.
    Padding both sets the same way changes no Hamming distance."""
    a = np.asarray(a)
    if a.ndim != 2:
        raise ValueError("pack_bits takes a 2-D array of 0 / 1 values")
    if a.dtype != np.bool_:
        if ((a != 0) & (a != 1)).any():
            raise ValueError("pack_bits takes bool or 0 / 1 values")
        a = a.astype(np.bool_)
    n, k = a.shape
    out = np.zeros((n, 4 * ((k + 31) // 32)), dtype=np.uint8)
    out[:, :(k + 7) // 8] = np.packbits(a, axis=1, bitorder="little")
    return out


def search_b1(query_points, reference_points, *, return_distances: bool = False, shards: int = 1,
              path: str = "auto", device: int = 0):
    """search() for packed binary points (see to_b1 / pack_bits) under Hamming distance (nns_search_b1_ex): the distances
    are the Hamming distances as fp32, V0's arithmetic on the bits widened to 0.0 / 1.0."""
    return _search_1nn(4, query_points, reference_points, return_distances, shards, path, device)


def _search_topk(q, r, kn, bf16, return_distances, shards, path, device, refs_soa, topk_mfma=False):
    if q.shape[1] != (r.shape[0] if refs_soa else r.shape[1]):
        raise ValueError("query and reference dimensionality differ")
    pt = _POINT_TYPES[int(bf16)]
    assert (pt.refs_soa or not refs_soa) and (pt.mfma_flags or not topk_mfma)
    m, k = q.shape
    k *= pt.k_mult   # (packed binary points: uint8 columns, k in bits)
    n = r.shape[1] if refs_soa else r.shape[0]
    idx = np.empty((m, max(kn, 0)), dtype=np.int32)
    dist = np.empty((m, max(kn, 0)), dtype=np.float32) if return_distances else None
    fn = getattr(lib, pt.search_name("topk"))
    _check(fn(k, m, n, q.ctypes.data, r.ctypes.data, kn, idx.ctypes.data, dist.ctypes.data if dist is not None else None,
              shards, _PATHS[path] | (NNS_REFS_SOA if refs_soa else 0) | (NNS_TOPK_MFMA if topk_mfma else 0), device),
           "nns_search_topk")
    return (idx, dist) if return_distances else idx


def search_topk(query_points, reference_points, kn: int, *, return_distances: bool = False, shards: int = 1,
                path: str = "auto", device: int = 0, refs_soa: bool = False, topk_mfma: bool = False):
    """The kn nearest references of every query (nns_search_f32_topk): int32 [m][kn] indices in ascending
    (V0 distance, index) order, -1 where fewer than kn references are selectable; optionally the fp32 distances
    (+INF in those slots).  ``shards`` > 1 rehearses the contiguous ref split merged with keys_topk_merge.
    topk_mfma: through the bound / flag / select path (NNS_TOPK_MFMA; 8 <= k <= 256), same results."""
    q = _as_f32(query_points, "query_points")
    r = _as_f32(reference_points, "reference_points")
    return _search_topk(q, r, kn, False, return_distances, shards, path, device, refs_soa, topk_mfma)


def search_topk_bf16(query_bits, reference_bits, kn: int, *, return_distances: bool = False, shards: int = 1,
                     path: str = "auto", device: int = 0, refs_soa: bool = False, topk_mfma: bool = False):
    """search_topk() for bf16 point sets given as uint16 bit patterns (nns_search_bf16_topk).  topk_mfma: NNS_TOPK_MFMA
    (32 <= k <= 256 for bf16 points)."""
    return _search_topk(_as_bf16_bits(query_bits), _as_bf16_bits(reference_bits), kn, True, return_distances, shards, path, device, refs_soa, topk_mfma)


def search_topk_f16(query_points, reference_points, kn: int, *, return_distances: bool = False, shards: int = 1,
                    path: str = "auto", device: int = 0, refs_soa: bool = False):
    """search_topk() for fp16 point sets (numpy float16 or uint16 bit patterns; nns_search_f16_topk)."""
    return _search_topk(to_f16_bits(query_points), to_f16_bits(reference_points), kn, 2, return_distances, shards, path,
                        device, refs_soa)


def search_topk_i8(query_points, reference_points, kn: int, *, return_distances: bool = False, shards: int = 1,
                   path: str = "auto", device: int = 0):
    """search_topk() for int8 point sets (numpy int8; nns_search_i8_topk)."""
    return _search_topk(to_i8(query_points), to_i8(reference_points), kn, 3, return_distances, shards, path, device, False)


def search_topk_u8(query_points, reference_points, kn: int, *, return_distances: bool = False, shards: int = 1,
                   path: str = "auto", device: int = 0, topk_mfma: bool = False):
    """search_topk() for uint8 point sets (numpy uint8; nns_search_u8_topk).  topk_mfma: NNS_TOPK_MFMA (32 <= k <= 256)."""
    return _search_topk(to_u8(query_points), to_u8(reference_points), kn, 5, return_distances, shards, path, device, False,
                        topk_mfma)


def search_topk_b1(query_points, reference_points, kn: int, *, return_distances: bool = False, shards: int = 1,
                   path: str = "auto", device: int = 0):
    """search_topk() for packed binary points (see to_b1 / pack_bits; nns_search_b1_topk)."""
    return _search_topk(to_b1(query_points), to_b1(reference_points), kn, 4, return_distances, shards, path, device, False)


def _search_range(q, r, radius2, bf16, return_distances, path, device, refs_soa, range_mfma=False):
    if q.shape[1] != (r.shape[0] if refs_soa else r.shape[1]):
        raise ValueError("query and reference dimensionality differ")
    pt = _POINT_TYPES[int(bf16)]
    assert (pt.refs_soa or not refs_soa) and (pt.mfma_flags or not range_mfma)
    m, k = q.shape
    k *= pt.k_mult   # (packed binary points: uint8 columns, k in bits)
    n = r.shape[1] if refs_soa else r.shape[0]
    lims = np.zeros(max(m, 0) + 1, dtype=np.int64)
    pidx = ctypes.POINTER(ctypes.c_int)()
    pdist = ctypes.POINTER(ctypes.c_float)()
    fn = getattr(lib, pt.search_name("range"))
    _check(fn(k, m, n, q.ctypes.data, r.ctypes.data, float(radius2), lims.ctypes.data, ctypes.byref(pidx),
              ctypes.byref(pdist) if return_distances else None,
              _PATHS[path] | (NNS_REFS_SOA if refs_soa else 0) | (NNS_RANGE_MFMA if range_mfma else 0),
              device), "nns_search_range")
    total = int(lims[-1])
    try:
        idx = np.ctypeslib.as_array(pidx, shape=(total,)).copy() if total else np.empty(0, np.int32)
        dist = None
        if return_distances:
            dist = np.ctypeslib.as_array(pdist, shape=(total,)).copy() if total else np.empty(0, np.float32)
    finally:
        _libc.free(pidx)
        if return_distances:
            _libc.free(pdist)
    return (lims, idx, dist) if return_distances else (lims, idx)


def search_range(query_points, reference_points, radius2: float, *, return_distances: bool = False,
                 path: str = "auto", device: int = 0, refs_soa: bool = False, range_mfma: bool = False):
    """Every reference within squared radius ``radius2`` of each query (nns_search_f32_range), in CSR form:
    (lims int64[m + 1], idx int32[lims[m]][, dist fp32[lims[m]]]); query i's hits are idx[lims[i]:lims[i + 1]] in
    ascending index order, with their V0 distances (d <= radius2, NaN / +INF never).  range_mfma: through the MFMA
    flag pass (NNS_RANGE_MFMA; 8 <= k <= 256), same results."""
    q = _as_f32(query_points, "query_points")
    r = _as_f32(reference_points, "reference_points")
    return _search_range(q, r, radius2, False, return_distances, path, device, refs_soa, range_mfma)


def search_range_bf16(query_bits, reference_bits, radius2: float, *, return_distances: bool = False,
                      path: str = "auto", device: int = 0, refs_soa: bool = False, range_mfma: bool = False):
    """search_range() for bf16 point sets given as uint16 bit patterns (nns_search_bf16_range).  range_mfma:
    NNS_RANGE_MFMA (32 <= k <= 256 for bf16 points)."""
    return _search_range(_as_bf16_bits(query_bits), _as_bf16_bits(reference_bits), radius2, True, return_distances, path, device, refs_soa, range_mfma)


def search_range_f16(query_points, reference_points, radius2: float, *, return_distances: bool = False,
                     path: str = "auto", device: int = 0, refs_soa: bool = False):
    """search_range() for fp16 point sets (numpy float16 or uint16 bit patterns; nns_search_f16_range)."""
    return _search_range(to_f16_bits(query_points), to_f16_bits(reference_points), radius2, 2, return_distances, path,
                         device, refs_soa)


def search_range_i8(query_points, reference_points, radius2: float, *, return_distances: bool = False,
                    path: str = "auto", device: int = 0):
    """search_range() for int8 point sets (numpy int8; nns_search_i8_range)."""
    return _search_range(to_i8(query_points), to_i8(reference_points), radius2, 3, return_distances, path, device, False)


def search_range_u8(query_points, reference_points, radius2: float, *, return_distances: bool = False,
                    path: str = "auto", device: int = 0, range_mfma: bool = False):
    """search_range() for uint8 point sets (numpy uint8; nns_search_u8_range).  range_mfma: NNS_RANGE_MFMA
    (32 <= k <= 256)."""
    return _search_range(to_u8(query_points), to_u8(reference_points), radius2, 5, return_distances, path, device, False,
                         range_mfma)


def search_range_b1(query_points, reference_points, radius2: float, *, return_distances: bool = False,
                    path: str = "auto", device: int = 0):
    """search_range() for packed binary points (see to_b1 / pack_bits; nns_search_b1_range): radius2 is compared with the
    Hamming distance."""
    return _search_range(to_b1(query_points), to_b1(reference_points), radius2, 4, return_distances, path, device, False)


# ---------------------------------------------------------------------------
# device-resident API (torch tensors are only the owners of device memory)
# ---------------------------------------------------------------------------
def _stream_ptr(stream) -> Optional[int]:
    if stream is None:
        import torch
        return torch.cuda.current_stream().cuda_stream or None
    return getattr(stream, "cuda_stream", stream) or None


def fill_uniform(t, seed: int, offset: int = 0, stream=None) -> None:
    """t[i] = synthetic uniform [0,1) value #(offset+i) of stream `seed` (same bits as
    oracle nns_rng_fill)."""
    _check(lib.nns_fill_uniform(t.data_ptr(), t.numel(), seed, offset, _stream_ptr(stream)), "nns_fill_uniform")


class Index:
    """One prepared, device-resident shard of reference points (nns_index)."""

    def __init__(self, refs, *, index_base: int = 0, path: str = "auto", profile: bool = False, stream=None,
                 soa: bool = False, filter_bf16: bool = False, filter_f32: bool = False,
                 filter_split_eager: bool = False, range_mfma: bool = False, topk_mfma: bool = False,
                 filter_i8pre: str = "auto", points=None):
        """refs: [n][k] (or, with soa=True, dimension-major [k][n]: NNS_REFS_SOA) on a HIP device.
        filter_f32: fp32 points through fp32 filter operands (NNS_FILTER_F32) instead of split-bf16 ones.
        filter_split_eager: the split operands' eager schedule at every depth (NNS_FILTER_SPLIT_EAGER).
        range_mfma: range searches of this index go through the MFMA flag pass (NNS_RANGE_MFMA).
        topk_mfma: top-K searches of this index go through the bound / flag / select path (NNS_TOPK_MFMA).
        filter_i8pre: "auto" | "off" | "force" — the int8 pre-pass of the 128-deep lazy filter (NNS_FILTER_I8PRE_*).
        A torch.uint8 [n][kb] tensor is a set of packed binary points (pack_bits' layout; kb % 4 == 0, 4-byte aligned):
        Hamming distance, self.k = 8 * kb bits, self.b1 is true, queries are uint8 [m][kb] likewise.
        points: None infers the point type from the tensor's dtype as above; "u8" takes a torch.uint8 [n][k] tensor as
        uint8 point values 0 .. 255 (self.u8 is true; range_mfma / topk_mfma at 32 <= k <= 256)."""
        import torch
        if refs.dtype not in (torch.float32, torch.bfloat16, torch.float16, torch.int8, torch.uint8) or refs.dim() != 2 \
                or not refs.is_contiguous() or not refs.is_cuda:
            raise ValueError("refs must be a contiguous fp32, bf16, fp16, int8 or uint8 (packed bits) [n][k] tensor on a HIP device")
        if points not in (None, "u8"):
            raise ValueError('points must be None (inferred from the dtype) or "u8"')
        if points == "u8" and refs.dtype != torch.uint8:
            raise ValueError('points="u8" takes a torch.uint8 tensor')
        code = 5 if points == "u8" else {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2, torch.int8: 3,
                                         torch.uint8: 4}[refs.dtype]
        self._pt = _POINT_TYPES[code]
        self.bf16, self.f16, self.i8, self.b1, self.u8 = (code == c for c in (1, 2, 3, 4, 5))
        if self.b1 and (refs.shape[1] % 4 != 0 or refs.data_ptr() % 4 != 0):
            raise ValueError("packed binary refs hold whole 32-bit words: kb % 4 == 0 and a 4-byte aligned data_ptr()")
        self.refs = refs  # keep alive: the index reads the original values
        self.n, self.k = (refs.shape[1], refs.shape[0]) if soa else refs.shape
        self.cols = self.k   # columns of a query tensor
        self.k *= self._pt.k_mult   # (packed binary points: bits)
        self.device = refs.device.index or 0
        flags = _PATHS[path] | (NNS_PROFILE if profile else 0) | (NNS_REFS_SOA if soa else 0) \
            | (NNS_FILTER_BF16 if filter_bf16 else 0) | (NNS_FILTER_F32 if filter_f32 else 0) \
            | (NNS_FILTER_SPLIT_EAGER if filter_split_eager else 0) | (NNS_RANGE_MFMA if range_mfma else 0) \
            | (NNS_TOPK_MFMA if topk_mfma else 0) | _I8PRE[filter_i8pre]
        self.flags = flags
        h = ctypes.c_void_p()
        create = getattr(lib, self._pt.index_name("create"))
        _check(create(ctypes.byref(h), self.device, self.k, self.n, refs.data_ptr(),
                      index_base, flags, _stream_ptr(stream)), "nns_index_create")
        self._h = h

    def filter_pre(self) -> bool:
        """Did the last search's filter run the int8 pre-pass kernel?  (nns_index_filter_pre: waits for the index's stream)"""
        ran = ctypes.c_int(0)
        _check(lib.nns_index_filter_pre(self._h, ctypes.byref(ran)), "nns_index_filter_pre")
        return bool(ran.value)

    def refresh(self, stream=None) -> None:
        _check(lib.nns_index_refresh(self._h, _stream_ptr(stream)), "nns_index_refresh")

    def search_keys(self, queries, keys=None, stream=None):
        """Packed (V0 distance, global index) int64 key per query (NNS_KEY_NONE if none)."""
        import torch
        if queries.dtype != self.refs.dtype or queries.dim() != 2 or not queries.is_contiguous():
            raise ValueError("queries must be a contiguous [m][k] tensor of the index's dtype")
        if queries.shape[1] != self.cols:
            raise ValueError("query dimensionality differs from the index")
        self._check_aligned(queries)
        m = queries.shape[0]
        if keys is None:
            keys = torch.empty(m, dtype=torch.int64, device=queries.device)
        fn = getattr(lib, self._pt.index_name("search"))
        _check(fn(self._h, m, queries.data_ptr(), keys.data_ptr(), _stream_ptr(stream)), "nns_index_search")
        return keys

    def search(self, queries, return_distances: bool = False, stream=None):
        keys = self.search_keys(queries, stream=stream)
        return keys_unpack(keys, return_distances=return_distances, stream=stream)

    def search_indices(self, queries, keys=None, idx=None, dist=None, stream=None):
        """nns_index_search_indices: keys AND unpacked int32 indices (and, if `dist` is given,
        distances) of a single-shard search in as few launches as the path allows."""
        import torch
        if queries.dtype != self.refs.dtype or queries.dim() != 2 or not queries.is_contiguous() \
                or queries.shape[1] != self.cols:
            raise ValueError("queries must be a contiguous [m][k] tensor of the index's dtype")
        self._check_aligned(queries)
        m = queries.shape[0]
        if keys is None:
            keys = torch.empty(m, dtype=torch.int64, device=queries.device)
        if idx is None:
            idx = torch.empty(m, dtype=torch.int32, device=queries.device)
        _check(lib.nns_index_search_indices(self._h, m, queries.data_ptr(), keys.data_ptr(), idx.data_ptr(),
                                            dist.data_ptr() if dist is not None else None, _stream_ptr(stream)),
               "nns_index_search_indices")
        return idx

    def search_topk_keys(self, queries, kn: int, keys=None, stream=None):
        """[m][kn] packed (V0 distance, global index) int64 keys, ascending; NNS_KEY_NONE pads short rows."""
        import torch
        if queries.dtype != self.refs.dtype or queries.dim() != 2 or not queries.is_contiguous() \
                or queries.shape[1] != self.cols:
            raise ValueError("queries must be a contiguous [m][k] tensor of the index's dtype")
        self._check_aligned(queries)
        m = queries.shape[0]
        if keys is None:
            keys = torch.empty((m, max(kn, 0)), dtype=torch.int64, device=queries.device)
        _check(lib.nns_index_search_topk(self._h, m, queries.data_ptr(), kn, keys.data_ptr(), _stream_ptr(stream)),
               "nns_index_search_topk")
        return keys

    def search_topk(self, queries, kn: int, return_distances: bool = False, stream=None):
        """The kn nearest refs of every query: int32 [m][kn] (-1 in unfilled slots), optionally fp32 distances."""
        keys = self.search_topk_keys(queries, kn, stream=stream)
        return keys_topk_unpack(keys, return_distances=return_distances, stream=stream)

    def topk_info(self) -> dict:
        """nns_index_topk_info: what the last top-K search did — path (1 exact K6, 2 MFMA-filtered K6m), flagged and
        examined (query, 32-ref block) pairs, queries whose flag row was filled.  Waits for the index's stream."""
        out = np.zeros(4, np.int64)
        _check(lib.nns_index_topk_info(self._h, out.ctypes.data, 4), "nns_index_topk_info")
        return dict(zip(("path", "flagged", "examined", "filled"), (int(v) for v in out)))

    def _check_aligned(self, queries):
        if self.b1 and queries.data_ptr() % 4 != 0:
            raise ValueError("packed binary queries must be 4-byte aligned")

    def _check_queries(self, queries):
        if queries.dtype != self.refs.dtype or queries.dim() != 2 or not queries.is_contiguous() \
                or queries.shape[1] != self.cols:
            raise ValueError("queries must be a contiguous [m][k] tensor of the index's dtype")
        self._check_aligned(queries)

    def range_count(self, queries, radius2: float, lims=None, stream=None):
        """Count pass of the range search: int64 lims [m + 1] (device); the fill's per-chunk offsets stay in the
        index."""
        import torch
        self._check_queries(queries)
        m = queries.shape[0]
        if lims is None:
            lims = torch.empty(m + 1, dtype=torch.int64, device=queries.device)
        _check(lib.nns_index_range_count(self._h, m, queries.data_ptr(), float(radius2), lims.data_ptr(),
                                         _stream_ptr(stream)), "nns_index_range_count")
        return lims

    def range_fill(self, queries, radius2: float, lims, total: Optional[int] = None, return_distances: bool = False,
                   idx=None, dist=None, stream=None):
        """Fill pass after range_count with the same queries and radius2: int32 idx [lims[m]] (and fp32 distances).
        total: lims[m] if the caller has read it (otherwise it is read here, after waiting for `stream`, where the
        count ran).  With no hits the buffers are empty and their null pointers are not written."""
        import torch
        self._check_queries(queries)
        m = queries.shape[0]
        if idx is None or (return_distances and dist is None):
            if total is None:
                if stream is not None:
                    stream.synchronize()   # (a torch stream: the read below runs on the current one)
                total = int(lims[-1].item())
            if idx is None:
                idx = torch.empty(total, dtype=torch.int32, device=queries.device)
            if return_distances and dist is None:
                dist = torch.empty(total, dtype=torch.float32, device=queries.device)
        _check(lib.nns_index_range_fill(self._h, m, queries.data_ptr(), float(radius2), lims.data_ptr(), idx.data_ptr(),
                                        dist.data_ptr() if dist is not None else None, _stream_ptr(stream)),
               "nns_index_range_fill")
        return (idx, dist) if return_distances else idx

    def search_range(self, queries, radius2: float, return_distances: bool = False, stream=None):
        """Every ref within squared radius radius2 of each query: (lims int64 [m + 1], idx int32 [lims[m]][, dist]),
        torch tensors on the device.  Counts, reads lims[m] (one wait for the count), allocates and fills."""
        lims = self.range_count(queries, radius2, stream=stream)
        if stream is not None:
            stream.synchronize()   # (a torch stream: the read below runs on the current one)
        total = int(lims[-1].item())
        out = self.range_fill(queries, radius2, lims, total=total, return_distances=return_distances, stream=stream)
        return (lims,) + out if return_distances else (lims, out)

    def range_info(self) -> dict:
        """nns_index_range_info: what the last range_count did — path (1 exact K7, 2 MFMA-filtered), flagged and
        examined (query, 32-ref block) pairs, total hits.  Waits for the index's stream."""
        out = np.zeros(4, np.int64)
        _check(lib.nns_index_range_info(self._h, out.ctypes.data, 4), "nns_index_range_info")
        return dict(zip(("path", "flagged", "examined", "hits"), (int(v) for v in out)))

    def stats(self) -> dict:
        st = nns_stats()
        _check(lib.nns_index_stats(self._h, ctypes.byref(st)), "nns_index_stats")
        d = st.asdict()
        # the filter's operand form the index uses: "split" (split-bf16, fp32 points by default), "fp32"
        # (NNS_FILTER_F32 or a depth without the split form), "bf16" (bf16 points / NNS_FILTER_BF16), "f16" (fp16 points),
        # "i8" (int8 and uint8 points: the int8 filter);
        # None: exact path
        form = ctypes.c_int(-1)
        _check(lib.nns_index_filter_form(self._h, ctypes.byref(form)), "nns_index_filter_form")
        d["filter_form"] = {-1: None, 0: "fp32", 1: "bf16", 2: "bf16", 3: "split", 4: "f16", 5: "i8"}[form.value]
        return d

    def near_ties(self) -> np.ndarray:
        """Query numbers of the last search that K5 decided among > 1 candidates within tau."""
        cnt = ctypes.c_int(0)
        _check(lib.nns_index_near_ties(self._h, None, 0, ctypes.byref(cnt)), "nns_index_near_ties")
        ids = np.empty(max(cnt.value, 1), dtype=np.int32)
        _check(lib.nns_index_near_ties(self._h, ids.ctypes.data, cnt.value, ctypes.byref(cnt)), "nns_index_near_ties")
        return np.sort(ids[:cnt.value])

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib.nns_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def warmup(device: int = 0) -> None:
    """nns_warmup: touch every kernel family once (code load, LDS opt-in, pool)."""
    _check(lib.nns_warmup(device), "nns_warmup")


def trim() -> int:
    """nns_trim: return the pooled device workspaces to the runtime; bytes released."""
    return int(lib.nns_trim())


def keys_min(inout, other, stream=None) -> None:
    _check(lib.nns_keys_min(inout.data_ptr(), other.data_ptr(), inout.numel(), _stream_ptr(stream)), "nns_keys_min")


def keys_unpack(keys, return_distances: bool = False, stream=None):
    import torch
    m = keys.numel()
    idx = torch.empty(m, dtype=torch.int32, device=keys.device)
    dist = torch.empty(m, dtype=torch.float32, device=keys.device) if return_distances else None
    _check(lib.nns_keys_unpack(keys.data_ptr(), m, idx.data_ptr(),
                               dist.data_ptr() if dist is not None else None, _stream_ptr(stream)),
           "nns_keys_unpack")
    return (idx, dist) if return_distances else idx


def keys_topk_merge(inout, other, stream=None) -> None:
    """inout[i] = the kn smallest keys of the ascending rows inout[i] and other[i] ([m][kn] int64 tensors)."""
    if inout.shape != other.shape or inout.dim() != 2:
        raise ValueError("keys_topk_merge: two [m][kn] key tensors of one shape")
    m, kn = inout.shape
    _check(lib.nns_keys_topk_merge(inout.data_ptr(), other.data_ptr(), m, kn, _stream_ptr(stream)), "nns_keys_topk_merge")


def keys_topk_unpack(keys, return_distances: bool = False, stream=None):
    """[m][kn] keys -> int32 indices (-1 for NNS_KEY_NONE) and, optionally, fp32 distances (+INF there)."""
    import torch
    if keys.dim() != 2:
        raise ValueError("keys_topk_unpack: an [m][kn] key tensor")
    m, kn = keys.shape
    idx = torch.empty((m, kn), dtype=torch.int32, device=keys.device)
    dist = torch.empty((m, kn), dtype=torch.float32, device=keys.device) if return_distances else None
    _check(lib.nns_keys_topk_unpack(keys.data_ptr(), m, kn, idx.data_ptr(),
                                    dist.data_ptr() if dist is not None else None, _stream_ptr(stream)),
           "nns_keys_topk_unpack")
    return (idx, dist) if return_distances else idx


def shard_range(n: int, shards: int, rank: int) -> Tuple[int, int]:
    """Contiguous ceil(n/shards) split of the refs, last shard takes the remainder
    (reference core.cu:781-791).  Returns (begin, count); count may be 0."""
    per = -(-n // shards)
    beg = rank * per
    cnt = max(0, min(per, n - beg))
    return beg, cnt


def comm_unique_id() -> bytes:
    """nns_comm_unique_id: the 128 bytes rank 0 hands to every rank (RCCL's ncclUniqueId)."""
    buf = ctypes.create_string_buffer(NNS_COMM_ID_BYTES)
    _check(lib.nns_comm_unique_id(buf, NNS_COMM_ID_BYTES), "nns_comm_unique_id")
    return buf.raw


class Comm:
    """One rank of the one-process-per-GPU exchange (nns_comm): ONE
    ncclAllReduce(ncclUint64, ncclMin) of the packed keys per search, issued by the library —
    the same call site nns_search_f32_multi uses.  Creation is collective over all ranks."""

    def __init__(self, unique_id: bytes, nranks: int, rank: int, device: int):
        h = ctypes.c_void_p()
        _check(lib.nns_comm_create(ctypes.byref(h), unique_id, len(unique_id), nranks, rank, device),
               "nns_comm_create")
        self._h = h
        self.nranks, self.rank, self.device = nranks, rank, device

    def size(self) -> int:
        return lib.nns_comm_size(self._h)

    def allreduce_min(self, keys, stream=None) -> None:
        _check(lib.nns_comm_allreduce_min(self._h, keys.data_ptr(), keys.numel(), _stream_ptr(stream)),
               "nns_comm_allreduce_min")

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib.nns_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def multi_last_exchange_ranks() -> int:
    """Ranks of the last grouped RCCL all-reduce a search_multi call completed (0: none / host merge)."""
    return int(lib.nns_multi_last_exchange_ranks())


def shutdown() -> None:
    """nns_shutdown: destroy the cached communicators of search_multi, trim the pool."""
    _check(lib.nns_shutdown(), "nns_shutdown")


def allreduce_min_keys(keys, group=None, comm: Optional[Comm] = None) -> None:
    """The cross-GPU exchange: ONE min all-reduce of the packed keys.  With `comm` the library
    issues it itself (ncclAllReduce(uint64, min) over xGMI, nns_comm_allreduce_min); without,
    it goes through torch.distributed (RCCL when the process group is 'nccl'; gloo in CPU
    tests).  Keys are < 2^63, so the signed int64 order torch reduces in is the unsigned key
    order and both give the same bits."""
    if comm is not None:
        comm.allreduce_min(keys)
        return
    import torch.distributed as dist
    if keys.is_cuda and dist.get_backend(group) == "gloo":
        # rehearsal on a box without one GPU per rank: same operator through the host
        h = keys.cpu()
        dist.all_reduce(h, op=dist.ReduceOp.MIN, group=group)
        keys.copy_(h)
        return
    dist.all_reduce(keys, op=dist.ReduceOp.MIN, group=group)
