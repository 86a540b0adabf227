"""CPU tests of the range (fixed-radius neighbour) boundary: the numpy range oracle the GPU tests use agrees with the
V0 oracle, the new C-ABI symbols are exported, arguments are validated before any device is touched, the launch
planner (nns_plan_range) keeps its invariants, and the GPU tests' case table (RANGE_CASES) reaches every K7 scan
instantiation."""
import ctypes
from collections import namedtuple

import numpy as np
import pytest
import torch

NNS_MAX_POINTS = 0x7FF00000
WS_BUDGET_BYTES = 256 << 20       # the range workspace's stated cap (include/nns.h)
LDS_BYTES = 160 * 1024
RANGE_SYMBOLS = ("nns_index_range_count", "nns_index_range_fill", "nns_search_f32_range", "nns_search_bf16_range",
                 "nns_plan_range")

# One case per (point type, load width, tile width) of range_scan_kernel<QT, VEC, T, FILL>; every case runs both the
# count (FILL = false) and the fill (FILL = true) instantiation, so the 20 cases reach all 40.  `offset` is the ref
# view's storage offset in elements (1: the pointer is not 4-element aligned, so the scan takes VEC = 1 although
# k % 4 == 0); qt / vec are what the planner and the launcher must pick for the shape.
RangeCase = namedtuple("RangeCase", "dtype k m n offset qt vec")
RANGE_CASES = [
    RangeCase("f32", 16, 40, 3000, 0, 16, 4),
    RangeCase("f32", 16, 40, 3000, 1, 16, 1),         # misaligned view of k % 4 == 0 refs
    RangeCase("f32", 32, 7, 3000, 0, 8, 4),           # seven queries: the tile shrinks to 8
    RangeCase("f32", 33, 8, 3000, 0, 8, 1),
    RangeCase("f32", 4096, 6, 1500, 0, 4, 4),         # the 64 KiB query tile holds 4 queries
    RangeCase("f32", 2049, 7, 1500, 0, 4, 1),
    RangeCase("f32", 8, 2, 3000, 0, 2, 4),
    RangeCase("f32", 8192, 3, 800, 1, 2, 1),
    RangeCase("f32", 16384, 2, 1000, 0, 1, 4),        # the documented k limit
    RangeCase("f32", 5, 1, 5000, 0, 1, 1),
    RangeCase("bf16", 32, 40, 3000, 0, 16, 4),
    RangeCase("bf16", 33, 40, 3000, 0, 16, 1),
    RangeCase("bf16", 40, 8, 3000, 0, 8, 4),
    RangeCase("bf16", 64, 6, 3000, 1, 8, 1),
    RangeCase("bf16", 4096, 5, 1500, 0, 4, 4),
    RangeCase("bf16", 33, 3, 3000, 0, 4, 1),
    RangeCase("bf16", 8192, 3, 800, 0, 2, 4),
    RangeCase("bf16", 3, 2, 5000, 0, 2, 1),
    RangeCase("bf16", 16384, 2, 1000, 0, 1, 4),
    RangeCase("bf16", 257, 1, 3000, 0, 1, 1),
]


def range_case_id(c):
    return f"{c.dtype}-k{c.k}-m{c.m}-n{c.n}-off{c.offset}"


def scan_vec(k, ptr, elem_bytes):
    """The scan's ref load width for refs at address ptr (launch_range_scan's rule, as K6's)."""
    return 4 if k % 4 == 0 and ptr % (4 * elem_bytes) == 0 else 1


def v0_all(q, r, chunk=256):
    """Every V0 distance [m][n]: d = 0; for t ascending d = d + fl(q - r)^2 in fp32 (numpy does not fuse), computed
    in query chunks with topk_oracle's arithmetic."""
    q = np.ascontiguousarray(q, np.float32)
    r = np.ascontiguousarray(r, np.float32)
    rt = np.ascontiguousarray(r.T)
    d = np.empty((q.shape[0], r.shape[0]), np.float32)
    with np.errstate(all="ignore"):
        for c0 in range(0, q.shape[0], chunk):
            qc = q[c0:c0 + chunk]
            acc = np.zeros((qc.shape[0], r.shape[0]), np.float32)
            for t in range(q.shape[1]):
                diff = qc[:, t:t + 1] - rt[t][None, :]
                acc = acc + diff * diff
            d[c0:c0 + chunk] = acc
    return d


def range_oracle(q, r, radius2, index_base=0):
    """(lims int64[m + 1], idx int32[lims[m]], dist fp32[lims[m]]): the refs with V0 distance <= radius2 (fp32,
    inclusive; NaN / +INF never), ascending index per query, with their distances."""
    d = v0_all(q, r)
    r2 = np.float32(radius2)
    with np.errstate(invalid="ignore"):
        hit = (d <= r2) & (d < np.float32(np.inf))
    counts = hit.sum(axis=1).astype(np.int64)
    lims = np.zeros(q.shape[0] + 1, np.int64)
    np.cumsum(counts, out=lims[1:])
    rows, cols = np.nonzero(hit)                     # row-major: ascending index within each query
    return lims, (cols + index_base).astype(np.int32), d[rows, cols].astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("case", ["random", "ties", "nonfinite"])
def test_range_oracle_matches_v0(orc, case):
    rng = np.random.default_rng(11)
    k, m, n = 5, 40, 300
    q = rng.random((m, k), dtype=np.float32)
    r = rng.random((n, k), dtype=np.float32)
    if case == "ties":
        r[50:120] = r[10]
        q[:5] = r[10]
    if case == "nonfinite":
        r[::7, 1] = np.nan
        r[1::7, 2] = np.inf
        r[2::7, 0] = -np.inf
        r[3::7, 4] = 3e19            # squares overflow to +INF
    with np.errstate(all="ignore"):
        want_idx, want_dist = orc.v0_search(q, r)
    # the smallest radius that holds each query's nearest ref: exactly the refs at that distance are hits
    for i in range(m):
        lims, idx, dist = range_oracle(q[i:i + 1], r, want_dist[i])
        assert idx[0] == want_idx[i]
        assert _bits(dist[0]) == _bits(want_dist[i])
        assert np.all(_bits(dist) == _bits(want_dist[i]))
        assert np.all(np.diff(idx) > 0)
    lims, idx, dist = range_oracle(q, r, 0.3)
    assert lims[0] == 0 and np.all(np.diff(lims) >= 0) and lims[-1] == len(idx) == len(dist)
    for i in range(0, m, 7):
        seg = slice(lims[i], lims[i + 1])
        assert np.all(np.diff(idx[seg]) > 0)
        for j, dj in zip(idx[seg], dist[seg]):
            assert _bits(dj) == _bits(orc.pair_distance(q[i], r[j]))
            assert dj <= np.float32(0.3)
        # every ref outside the segment is farther (or non-finite)
        outside = np.setdiff1d(np.arange(n), idx[seg])
        for j in outside[::11]:
            dj = orc.pair_distance(q[i], r[j])
            assert not (dj <= np.float32(0.3))
    if case == "ties":
        lims, idx, _ = range_oracle(q[:1], r, 0.0)
        assert idx.tolist() == [10] + list(range(50, 120))
    if case == "nonfinite":
        lims, idx, _ = range_oracle(q, r, np.inf)
        bad = set(range(0, n, 7)) | set(range(1, n, 7)) | set(range(2, n, 7)) | set(range(3, n, 7))
        assert not (set(idx.tolist()) & bad)
        assert np.all(np.diff(lims) == n - len(bad))


def test_range_oracle_boundaries():
    q = np.zeros((2, 1), np.float32)
    q[1, 0] = 100.0
    r = np.array([[1.0], [2.0], [-1.0], [np.nan], [0.0]], np.float32)
    lims, idx, dist = range_oracle(q, r, 1.0, index_base=10)
    assert lims.tolist() == [0, 3, 3]
    assert idx.tolist() == [10, 12, 14] and dist.tolist() == [1.0, 1.0, 0.0]
    below = np.nextafter(np.float32(1.0), np.float32(0.0))        # a radius one ulp short of d = 1
    lims, idx, _ = range_oracle(q[:1], r, below)
    assert idx.tolist() == [4]
    lims, idx, _ = range_oracle(q, r, np.inf)
    assert lims.tolist() == [0, 4, 8]                                 # the NaN ref never


def test_range_symbols_exported(pkg):
    raw = ctypes.CDLL(pkg.LIB_PATH)
    for name in RANGE_SYMBOLS:
        assert name in pkg.ABI_SYMBOLS
        assert getattr(raw, name) is not None


def _whole(L, fn, k, m, n, q, r, radius2, lims, flags=0, idx=True):
    pidx = ctypes.POINTER(ctypes.c_int)()
    pdist = ctypes.POINTER(ctypes.c_float)()
    rc = fn(k, m, n, q, r, radius2, lims, ctypes.byref(pidx) if idx else None, ctypes.byref(pdist), flags, 0)
    assert not pidx and not pdist          # left NULL on every error
    return rc


def test_range_argument_validation_without_device(pkg):
    L = pkg.lib
    q = np.zeros((4, 3), np.float32)
    lims = np.zeros(5, np.int64)
    qp, lp = q.ctypes.data, lims.ctypes.data
    for fn in (L.nns_search_f32_range, L.nns_search_bf16_range):
        assert _whole(L, fn, 3, 0, 4, qp, qp, 1.0, lp) == 1
        assert _whole(L, fn, 3, -1, 4, qp, qp, 1.0, lp) == 1
        assert _whole(L, fn, 3, 4, 0, qp, qp, 1.0, lp) == 1
        assert _whole(L, fn, 0, 4, 4, qp, qp, 1.0, lp) == 1
        assert _whole(L, fn, -2, 4, 4, qp, qp, 1.0, lp) == 1
        assert _whole(L, fn, 3, 4, 4, None, qp, 1.0, lp) == 1
        assert _whole(L, fn, 3, 4, 4, qp, None, 1.0, lp) == 1
        assert _whole(L, fn, 3, 4, 4, qp, qp, 1.0, None) == 1
        assert _whole(L, fn, 3, 4, 4, qp, qp, 1.0, lp, idx=False) == 1
        assert _whole(L, fn, 3, 4, 4, qp, qp, float("nan"), lp) == 1
        assert _whole(L, fn, 3, 4, 4, qp, qp, -1.0, lp) == 1
        assert _whole(L, fn, 3, 4, 4, qp, qp, -1e-30, lp) == 1
        assert b"radius2" in L.nns_last_error()
        assert _whole(L, fn, 3, 4, NNS_MAX_POINTS + 1, qp, qp, 1.0, lp) == 1
        assert b"NNS_MAX_POINTS" in L.nns_last_error()
        assert _whole(L, fn, 3, NNS_MAX_POINTS + 1, 4, qp, qp, 1.0, lp) == 1
        # flags other than auto / exact / dimension-major refs / profiling
        for flags in (2, 3, 32, 128, 256, 512, 1 << 30):
            assert _whole(L, fn, 3, 4, 4, qp, qp, 1.0, lp, flags=flags) == 5, flags
        # k beyond the exact path's query tile
        assert _whole(L, fn, 16385, 4, 4, qp, qp, 1.0, lp) == 5
    # split API entry points: no index / null buffers
    assert L.nns_index_range_count(None, 4, qp, 1.0, lp, None) == 1
    assert L.nns_index_range_fill(None, 4, qp, 1.0, lp, qp, None, None) == 1
    out = np.zeros(6, np.int32)
    assert L.nns_plan_range(3, 4, 4, 0, out.ctypes.data, 5) == 1
    assert L.nns_plan_range(3, 4, 4, 0, None, 6) == 1
    assert L.nns_plan_range(0, 4, 4, 0, out.ctypes.data, 6) == 1
    assert L.nns_plan_range(3, 0, 4, 0, out.ctypes.data, 6) == 1
    assert L.nns_plan_range(3, 4, 0, 0, out.ctypes.data, 6) == 1
    assert L.nns_plan_range(3, NNS_MAX_POINTS + 1, 4, 0, out.ctypes.data, 6) == 1
    assert L.nns_plan_range(16385, 4, 4, 0, out.ctypes.data, 6) == 5


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device error path")
def test_range_valid_call_without_device_is_nodevice(pkg):
    q = np.zeros((4, 3), np.float32)
    lims = np.zeros(5, np.int64)
    for fn in (pkg.lib.nns_search_f32_range, pkg.lib.nns_search_bf16_range):
        assert _whole(pkg.lib, fn, 3, 4, 4, q.ctypes.data, q.ctypes.data, 0.5, lims.ctypes.data) == 4
        assert _whole(pkg.lib, fn, 3, 4, 4, q.ctypes.data, q.ctypes.data, float("inf"), lims.ctypes.data,
                      flags=64 | 16 | 1) == 4
    assert _whole(pkg.lib, pkg.lib.nns_search_f32_range, 3, 4, 4, q.ctypes.data, q.ctypes.data, -0.0,
                  lims.ctypes.data) == 4                 # -0.0 counts as 0: valid
    with pytest.raises(pkg.NNSError) as e:
        pkg.search_range(q, q, 1.0)
    assert e.value.status == 4


def _plan_grid():
    for k in (1, 3, 16, 128, 1024, 1025, 4096, 16384):
        for m in (1, 2, 3, 9, 64, 513, 4096, 65536, 1 << 20, 1 << 26, NNS_MAX_POINTS):
            for n in (1, 7, 1000, 70000, 1 << 20, 1 << 24, NNS_MAX_POINTS):
                yield k, m, n


def test_plan_range_invariants(pkg):
    for k, m, n in _plan_grid():
        for bf16 in (False, True):
            p = pkg.plan_range(k, m, n, bf16=bf16)
            qt, chunks, per = p["queries_per_wg"], p["chunks"], p["per"]
            where = (k, m, n, bf16, p)
            assert qt >= 1 and chunks >= 1 and per >= 1, where
            assert chunks * per >= n, where
            assert (chunks - 1) * per < n, where                       # every chunk non-empty
            assert chunks == 1 or per % 256 == 0, where                # whole rounds
            assert p["workgroups"] == min(-(-m // qt) * chunks, 0x7FFFFFFF), where
            assert p["lds_bytes"] <= LDS_BYTES, where
            assert qt * k * 4 <= 64 * 1024, where
            assert 0 <= p["ws_bytes"] <= WS_BUDGET_BYTES, where
            if chunks > 1:
                assert p["ws_bytes"] >= m * chunks * 4, where
            assert qt == 1 or qt // 2 < m, where


def test_plan_range_fills_the_chip(pkg):
    for k in (3, 16, 128, 1024):
        p = pkg.plan_range(k, 1, 1 << 20)
        assert p["workgroups"] >= 256, (k, p)
    for k, m in ((3, 1024), (16, 1024), (128, 4096)):
        p = pkg.plan_range(k, m, 1 << 20)
        assert p["workgroups"] >= 1024, (k, m, p)


def test_plan_range_rejects_beyond_exact_path(pkg):
    with pytest.raises(pkg.NNSError) as e:
        pkg.plan_range(16385, 4, 4)
    assert e.value.status == 5


def test_range_cases_reach_every_instantiation(pkg):
    # every case gets the tile width and load width it claims, and each covers a (T, VEC, QT) no other case does
    reached = []
    for c in RANGE_CASES:
        esz = 2 if c.dtype == "bf16" else 4
        p = pkg.plan_range(c.k, c.m, c.n, bf16=c.dtype == "bf16")
        assert p["queries_per_wg"] == c.qt, (c, p)
        assert scan_vec(c.k, 256 + c.offset * esz, esz) == c.vec, c   # (device allocations are 256-byte aligned)
        reached.append((c.dtype, c.vec, c.qt))
    want = {(t, v, q) for t in ("f32", "bf16") for v in (4, 1) for q in (16, 8, 4, 2, 1)}
    assert set(reached) == want
    assert len(reached) == len(want) == 20
