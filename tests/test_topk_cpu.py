"""CPU tests of the top-K (k nearest neighbours) boundary: the numpy oracle the GPU tests use agrees with the V0
oracle, the new C-ABI symbols are exported, arguments are validated before any device is touched, the launch
planner (nns_plan_topk) keeps its invariants, and the GPU tests' scan table (SCAN_CASES) reaches every scan kernel."""
import ctypes
from collections import namedtuple

import numpy as np
import pytest
import torch

NNS_MAX_POINTS = 0x7FF00000
WS_BUDGET_BYTES = 256 << 20       # the split workspace's stated cap (include/nns.h)
LDS_BYTES = 160 * 1024

# One case per instantiation of topk_scan_kernel<QT, VEC, T>: 5 tile widths x VEC in {4, 1} x {fp32, bf16}.
# `offset` is the ref view's storage offset in elements (1: the pointer is not 4-element aligned, so the scan
# takes VEC = 1 although k % 4 == 0); qt / vec are what the planner and the launcher must pick for the shape.
# test_topk_edges_gpu.py runs every case against the oracle; test_scan_cases_reach_every_instantiation below
# guards, without a device, that the table still reaches all 20.
ScanCase = namedtuple("ScanCase", "dtype k m n kn offset qt vec")
SCAN_CASES = [
    ScanCase("f32", 16, 40, 3000, 16, 0, 16, 4),
    ScanCase("f32", 16, 40, 3000, 16, 1, 16, 1),       # misaligned view of k % 4 == 0 refs
    ScanCase("f32", 32, 21, 3000, 17, 0, 8, 4),        # kn = 17: the QT = 16 / 8 switch
    ScanCase("f32", 33, 13, 3000, 64, 0, 8, 1),
    ScanCase("f32", 4096, 6, 1500, 32, 0, 4, 4),       # the 64 KiB query tile holds 4 queries
    ScanCase("f32", 2049, 7, 1500, 8, 0, 4, 1),
    ScanCase("f32", 8, 2, 3000, 256, 0, 2, 4),         # two queries: the tile shrinks to m
    ScanCase("f32", 8192, 3, 800, 5, 1, 2, 1),
    ScanCase("f32", 16384, 2, 1000, 3, 0, 1, 4),       # the documented k limit
    ScanCase("f32", 5, 1, 5000, 100, 0, 1, 1),
    ScanCase("bf16", 32, 40, 3000, 16, 0, 16, 4),
    ScanCase("bf16", 33, 40, 3000, 1, 0, 16, 1),
    ScanCase("bf16", 40, 33, 3000, 25, 0, 8, 4),
    ScanCase("bf16", 64, 24, 3000, 255, 1, 8, 1),
    ScanCase("bf16", 4096, 5, 1500, 64, 0, 4, 4),
    ScanCase("bf16", 33, 3, 3000, 20, 0, 4, 1),
    ScanCase("bf16", 8192, 3, 800, 9, 0, 2, 4),
    ScanCase("bf16", 3, 2, 5000, 3, 0, 2, 1),
    ScanCase("bf16", 16384, 2, 1000, 2, 0, 1, 4),
    ScanCase("bf16", 257, 1, 3000, 7, 0, 1, 1),
]


def scan_case_id(c):
    return f"{c.dtype}-k{c.k}-m{c.m}-n{c.n}-kn{c.kn}-off{c.offset}"


def scan_vec(k, ptr, elem_bytes):
    """The scan's ref load width for refs at address ptr (launch_topk_scan's rule)."""
    return 4 if k % 4 == 0 and ptr % (4 * elem_bytes) == 0 else 1


def topk_oracle(q, r, kn, chunk=64):
    """(idx int32[m][kn], dist fp32[m][kn]) by V0's arithmetic: d = 0; for t ascending d = d + fl(q - r)^2 in fp32
    (numpy does not fuse), non-finite distances dropped, ordered by (distance, index); short rows -1 / +INF."""
    q = np.ascontiguousarray(q, np.float32)
    r = np.ascontiguousarray(r, np.float32)
    m, k = q.shape
    n = r.shape[0]
    rt = np.ascontiguousarray(r.T)
    idx = np.full((m, kn), -1, np.int32)
    dist = np.full((m, kn), np.inf, np.float32)
    take = min(kn, n)
    with np.errstate(all="ignore"):
        for c0 in range(0, m, chunk):
            qc = q[c0:c0 + chunk]
            d = np.zeros((qc.shape[0], n), np.float32)
            for t in range(k):
                diff = qc[:, t:t + 1] - rt[t][None, :]
                d = d + diff * diff
            order = np.argsort(d, axis=1, kind="stable")[:, :take]    # NaN / INF sort last; ties by index
            dv = np.take_along_axis(d, order, axis=1)
            ok = np.isfinite(dv)
            idx[c0:c0 + chunk, :take] = np.where(ok, order, -1)
            dist[c0:c0 + chunk, :take] = np.where(ok, dv, np.float32(np.inf))
    return idx, dist


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("case", ["random", "ties", "nonfinite"])
def test_numpy_oracle_matches_v0(orc, case):
    rng = np.random.default_rng(7)
    k, m, n = 5, 40, 300
    q = rng.random((m, k), dtype=np.float32)
    r = rng.random((n, k), dtype=np.float32)
    if case == "ties":
        r[50:120] = r[10]
        q[:5] = r[10]
        r[200:] = r[3]
    if case == "nonfinite":
        r[::7, 1] = np.nan
        r[1::7, 2] = np.inf
        r[2::7, 0] = -np.inf
        r[3::7, 4] = 3e19            # squares overflow to +INF
    idx, dist = topk_oracle(q, r, 12)
    with np.errstate(all="ignore"):
        want_idx, want_dist = orc.v0_search(q, r)
    assert np.array_equal(idx[:, 0], want_idx)
    assert np.array_equal(_bits(dist[:, 0]), _bits(want_dist))
    for i in range(0, m, 7):
        for s in range(12):
            if idx[i, s] < 0:
                continue
            assert _bits(dist[i, s]) == _bits(orc.pair_distance(q[i], r[idx[i, s]]))
        ok = idx[i] >= 0
        keys = [(float(d), int(j)) for d, j in zip(dist[i][ok], idx[i][ok])]
        assert keys == sorted(keys)
    if case == "ties":
        assert list(idx[0]) == [10] + list(range(50, 61))
    if case == "nonfinite":
        bad = set(range(0, n, 7)) | set(range(1, n, 7)) | set(range(2, n, 7)) | set(range(3, n, 7))
        assert not (set(idx.ravel().tolist()) & bad)


def test_numpy_oracle_pads_short_rows():
    q = np.zeros((2, 3), np.float32)
    r = np.array([[1, 0, 0], [np.nan, 0, 0], [0, 2, 0]], np.float32)
    idx, dist = topk_oracle(q, r, 5)
    assert idx.tolist() == [[0, 2, -1, -1, -1]] * 2
    assert np.isinf(dist[:, 2:]).all() and dist[0, 1] == 4.0


def test_topk_symbols_exported(pkg):
    raw = ctypes.CDLL(pkg.LIB_PATH)
    for name in ("nns_index_search_topk", "nns_keys_topk_merge", "nns_keys_topk_unpack", "nns_search_f32_topk",
                 "nns_search_bf16_topk", "nns_plan_topk"):
        assert name in pkg.ABI_SYMBOLS
        assert getattr(raw, name) is not None


def test_topk_argument_validation_without_device(pkg):
    L = pkg.lib
    q = np.zeros((4, 3), np.float32)
    idx = np.zeros(4 * 300, np.int32)
    qp, ip = q.ctypes.data, idx.ctypes.data
    assert L.nns_search_f32_topk(3, 4, 4, qp, qp, 0, ip, None, 1, 0, 0) == 1
    assert L.nns_search_f32_topk(3, 4, 4, qp, qp, -3, ip, None, 1, 0, 0) == 1
    assert L.nns_search_f32_topk(3, 4, 4, qp, qp, 257, ip, None, 1, 0, 0) == 5
    assert b"above 256" in L.nns_last_error()
    assert L.nns_search_bf16_topk(3, 4, 4, qp, qp, 257, ip, None, 1, 0, 0) == 5
    assert L.nns_search_f32_topk(3, 0, 4, qp, qp, 4, ip, None, 1, 0, 0) == 1
    assert L.nns_search_f32_topk(3, -1, 4, qp, qp, 4, ip, None, 1, 0, 0) == 1
    assert L.nns_search_f32_topk(3, 4, 0, qp, qp, 4, ip, None, 1, 0, 0) == 1
    assert L.nns_search_f32_topk(0, 4, 4, qp, qp, 4, ip, None, 1, 0, 0) == 1
    assert L.nns_search_f32_topk(3, 4, 4, qp, qp, 4, None, None, 1, 0, 0) == 1
    assert L.nns_search_f32_topk(3, 4, 4, None, qp, 4, ip, None, 1, 0, 0) == 1
    assert L.nns_search_f32_topk(3, 4, NNS_MAX_POINTS + 1, qp, qp, 4, ip, None, 1, 0, 0) == 1
    assert b"NNS_MAX_POINTS" in L.nns_last_error()
    assert L.nns_search_bf16_topk(3, NNS_MAX_POINTS + 1, 4, qp, qp, 4, ip, None, 1, 0, 0) == 1
    # flags other than auto / exact / dimension-major refs / profiling
    for flags in (2, 32, 128, 256, 512):
        assert L.nns_search_f32_topk(3, 4, 4, qp, qp, 4, ip, None, 1, flags, 0) == 5, flags
    # k beyond the exact path's query tile
    assert L.nns_search_f32_topk(16385, 4, 4, qp, qp, 4, ip, None, 1, 0, 0) == 5
    # split API entry points: no index / null buffers
    assert L.nns_index_search_topk(None, 4, qp, 4, ip, None) == 1
    assert L.nns_keys_topk_merge(None, ip, 4, 4, None) == 1
    assert L.nns_keys_topk_merge(ip, ip, 4, 0, None) == 1
    assert L.nns_keys_topk_merge(ip, ip, 4, 257, None) == 5
    assert L.nns_keys_topk_unpack(ip, 4, 4, None, None, None) == 1
    assert L.nns_keys_topk_unpack(ip, 0, 4, ip, None, None) == 1
    assert L.nns_keys_topk_unpack(ip, 4, 257, ip, None, None) == 5
    out = np.zeros(6, np.int32)
    assert L.nns_plan_topk(3, 4, 4, 0, 0, out.ctypes.data, 6) == 1
    assert L.nns_plan_topk(3, 4, 4, 257, 0, out.ctypes.data, 6) == 5
    assert L.nns_plan_topk(3, 4, 4, 4, 0, out.ctypes.data, 5) == 1
    assert L.nns_plan_topk(3, 4, 4, 4, 0, None, 6) == 1
    assert L.nns_plan_topk(3, NNS_MAX_POINTS + 1, 4, 4, 0, out.ctypes.data, 6) == 1


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device error path")
def test_topk_valid_call_without_device_is_nodevice(pkg):
    q = np.zeros((4, 3), np.float32)
    idx = np.zeros(4 * 8, np.int32)
    assert pkg.lib.nns_search_f32_topk(3, 4, 4, q.ctypes.data, q.ctypes.data, 8, idx.ctypes.data, None, 1, 0, 0) == 4
    assert pkg.lib.nns_search_bf16_topk(3, 4, 4, q.ctypes.data, q.ctypes.data, 8, idx.ctypes.data, None, 2, 64, 0) == 4
    with pytest.raises(pkg.NNSError) as e:
        pkg.search_topk(q, q, 3)
    assert e.value.status == 4


def _plan_grid():
    for k in (1, 3, 16, 128, 1024, 16384):
        for m in (1, 3, 64, 513, 4096, 65536, 1 << 20):
            for n in (1, 7, 1000, 70000, 1 << 20, 1 << 24):
                for kn in (1, 2, 10, 64, 100, 256):
                    yield k, m, n, kn


def test_plan_topk_invariants(pkg):
    for k, m, n, kn in _plan_grid():
        for bf16 in (False, True):
            p = pkg.plan_topk(k, m, n, kn, bf16=bf16)
            qt, splits, per = p["queries_per_wg"], p["splits"], p["per"]
            where = (k, m, n, kn, bf16, p)
            assert qt >= 1 and splits >= 1 and per >= 1, where
            assert splits * per >= n, where
            assert (splits - 1) * per < n, where                      # every split non-empty
            assert p["workgroups"] == -(-m // qt) * splits, where
            assert p["lds_bytes"] <= LDS_BYTES, where
            assert qt * k * 4 <= 64 * 1024, where
            assert p["ws_keys"] * 8 <= WS_BUDGET_BYTES, where
            assert p["ws_keys"] == (splits * m * kn if splits > 1 else 0), where


def test_plan_topk_fills_the_chip_for_one_query(pkg):
    for k in (3, 16, 128):
        for kn in (1, 10, 100, 256):
            p = pkg.plan_topk(k, 1, 1 << 20, kn)
            assert p["workgroups"] >= 256, (k, kn, p)


def test_plan_topk_rejects_beyond_exact_path(pkg):
    with pytest.raises(pkg.NNSError) as e:
        pkg.plan_topk(16385, 4, 4, 4)
    assert e.value.status == 5


def test_scan_cases_reach_every_instantiation(pkg):
    # every case gets the tile width and load width it claims, and each covers a (T, VEC, QT) no other case does
    reached = []
    for c in SCAN_CASES:
        esz = 2 if c.dtype == "bf16" else 4
        p = pkg.plan_topk(c.k, c.m, c.n, c.kn, bf16=c.dtype == "bf16")
        assert p["queries_per_wg"] == c.qt, (c, p)
        assert scan_vec(c.k, 256 + c.offset * esz, esz) == c.vec, c   # (device allocations are 256-byte aligned)
        reached.append((c.dtype, c.vec, c.qt))
    want = {(t, v, q) for t in ("f32", "bf16") for v in (4, 1) for q in (16, 8, 4, 2, 1)}
    assert set(reached) == want
    assert len(reached) == len(want) == 20
