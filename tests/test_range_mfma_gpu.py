"""GPU tests of the MFMA-filtered range search (NNS_RANGE_MFMA, K7m): lims, indices and distance bits equal to the numpy
range oracle of test_range_cpu.py on every shape, through the split API of a flagged index and the whole call — a grid
over k, both ref image layouts, several ring slots / splits / chunks, the inclusive boundary, bounds on the number of
flagged blocks derived from the threshold's model, tightly clustered and re-scaled data, non-finite queries and refs,
index options, the count / fill contract, determinism, query batches and the caller's stream."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_range_cpu import range_oracle, v0_all  # noqa: E402
from test_range_gpu import _assert_same, _radii  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
INF = float("inf")
EXACT, MFMA = 1, 2
SPLIT_EAGER = 2048                                       # NNS_FILTER_SPLIT_EAGER


def _rand(seed, *shape):
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(out):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _search(ix, qd, radius2):
    """((lims, idx, dist) on the host, range_info of the count) of one split-API range search."""
    out = ix.search_range(qd, radius2, return_distances=True)
    return _host(out), ix.range_info()


# ---- 1. a grid over k -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 16, 24, 64, 100, 128, 200, 256])
def test_grid(pkg, k):
    m, n = 130, 2999
    q = _rand(10 + k, m, k)
    r = _rand(20 + k, n, k)
    r[100:140] = r[7]                                    # a run of equal distances for every query
    radii = _radii(v0_all(q, r), n)
    ix = pkg.Index(_dev(r), range_mfma=True)
    qd = _dev(q)
    for radius2 in radii:
        want = range_oracle(q, r, radius2)
        got, info = _search(ix, qd, radius2)
        _assert_same(got, want, f"split k={k} r2={radius2}")
        assert info["path"] == (EXACT if radius2 == INF else MFMA), (radius2, info)   # +INF takes K7
        assert info["hits"] == want[0][-1]
        if radius2 != INF:
            assert info["examined"] == m * pkg.plan_range_mfma(k, m, n)["blocks_per_query"]
            assert ix.stats()["path"] == MFMA
        _assert_same(pkg.search_range(q, r, radius2, return_distances=True, range_mfma=True), want,
                     f"whole k={k} r2={radius2}")
    ix.close()


# ---- 2. both image layouts ------------------------------------------------------------------------------------
@pytest.mark.parametrize("eager", [False, True], ids=["default", "eager"])
@pytest.mark.parametrize("k", [64, 128])
def test_both_image_layouts(pkg, k, eager):
    m, n = 70, 5000
    lazy_depth = pkg.plan_filter(k, 65536, 1 << 20, schedule=True)["lazy"] == 1
    layout = pkg.plan_range_mfma(k, m, n, SPLIT_EAGER if eager else 0)["layout"]
    assert layout == int(lazy_depth and not eager)
    if k == 128:
        assert layout == int(not eager)                  # the lazy depth: both layouts are reached
    q = _rand(31 + k, m, k)
    r = _rand(32 + k, n, k)
    radius2 = _radii(v0_all(q, r), n)[2]
    ix = pkg.Index(_dev(r), range_mfma=True, filter_split_eager=eager)
    got, info = _search(ix, _dev(q), radius2)
    _assert_same(got, range_oracle(q, r, radius2), f"k={k} eager={eager}")
    assert info["path"] == MFMA
    ix.close()


# ---- 3. several ring slots, splits and chunks -----------------------------------------------------------------
def test_slots_splits_chunks_and_block_edges(pkg):
    k, m, n = 16, 600, 70001                             # two query groups of 512; 69 flag words: two chunks
    p = pkg.plan_range_mfma(k, m, n)
    assert p["grid_x"] == 2 and p["grid_y"] > 1
    assert p["blocks_per_query"] * 32 > n + 31           # the last block that holds refs is partly padding
    q = _rand(41, m, k)
    r = _rand(42, n, k)
    for i, j in enumerate((0, 31, 32, n - 1, n - 9, 2047 * 32 + 5, 2048 * 32)):
        r[j] = q[7 * i]                                  # exact duplicates at block edges, chunk edge, last block
        r[j][0] += np.float32(1e-3)
    d = v0_all(q, r)
    radius2 = _radii(d, n)[1]                            # about 3 hits per query
    want = range_oracle(q, r, radius2)
    assert 2 * m < want[0][-1] < 6 * m
    ix = pkg.Index(_dev(r), range_mfma=True)
    got, info = _search(ix, _dev(q), radius2)
    _assert_same(got, want, "edges")
    assert info["path"] == MFMA and 0 < info["flagged"] < info["examined"] // 4
    for j in (0, 31, 32, n - 1, n - 9):
        assert j in got[1].tolist()
    ix.close()


# ---- 4. the inclusive boundary --------------------------------------------------------------------------------
def test_radius_is_inclusive_and_next_float_excluded(pkg):
    k, m, n = 16, 64, 5000
    q = _rand(51, m, k)
    r = _rand(52, n, k)
    d = v0_all(q, r)
    ix = pkg.Index(_dev(r), range_mfma=True)
    qd = _dev(q)
    for i in (0, 7, 63):
        j = int(np.argsort(d[i])[50])
        radius2 = float(d[i, j])
        at, info = _search(ix, qd, radius2)
        assert info["path"] == MFMA
        assert j in at[1][at[0][i]:at[0][i + 1]].tolist()                # at exactly radius2: in
        below = float(np.nextafter(np.float32(radius2), np.float32(0)))
        short, info = _search(ix, qd, below)
        assert info["path"] == MFMA
        assert j not in short[1][short[0][i]:short[0][i + 1]].tolist()   # one ulp short: out
        _assert_same(at, range_oracle(q, r, radius2), "inclusive")
        _assert_same(short, range_oracle(q, r, below), "next float")
    ix.close()


# ---- 5. the number of flagged blocks lies between the model's bounds ------------------------------------------
def test_flag_bounds(pkg):
    """Every block holding a hit is flagged, and a flagged block holds a ref with d <= radius2 + 2 tau(radius2 - |x'|^2)
    (the threshold is a + 1.002 tau(a) and a score lies within tau / 2 of d - |x'|^2; the
    2^-22 (radius2 + |x'|^2) term is below a thousandth of tau here).  Norms of the centred points are recomputed
    in fp64 around the fp32-rounded column mean; 1e-5 relative on the upper radius covers the mean's rounding."""
    k, m, n = 64, 128, 20000
    q = _rand(61, m, k)
    r = _rand(62, n, k)
    d = v0_all(q, r)
    radius2 = float(np.sort(d.ravel())[10 * m])          # about 10 hits per query
    kt = pkg.plan_range_mfma(k, m, n)["kt"]
    c = r.astype(np.float64).mean(axis=0).astype(np.float32)
    qn = ((q - c).astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
    ymax2 = float(((r - c).astype(np.float64) ** 2).sum(axis=1).max().astype(np.float32))
    nblk = -(-n // 32)
    dpad = np.full((m, nblk * 32), np.inf, np.float32)
    dpad[:, :n] = d
    bmin = dpad.reshape(m, nblk, 32).min(axis=2)         # the nearest ref of every (query, block)
    lo = int((bmin <= np.float32(radius2)).sum())
    hi = 0
    for i in range(m):
        c0, c1, x2 = pkg.tau_consts(kt, float(qn[i]), ymax2, 3)
        tau = c0 + c1 * max(radius2 - float(qn[i]) + x2, 0.0)
        hi += int((bmin[i].astype(np.float64) <= (radius2 + 2.0 * tau) * (1.0 + 1e-5)).sum())
    ix = pkg.Index(_dev(r), range_mfma=True)
    got, info = _search(ix, _dev(q), radius2)
    _assert_same(got, range_oracle(q, r, radius2), "flag bounds")
    print(f"flagged {info['flagged']} of {info['examined']} (lo {lo}, hi {hi})")
    assert info["path"] == MFMA and info["examined"] == m * pkg.plan_range_mfma(k, m, n)["blocks_per_query"]
    assert lo <= info["flagged"] <= hi, (lo, info, hi)
    assert hi < m * nblk // 2                            # (the bound says something: far from "everything")
    ix.close()


# ---- 6. a tight cluster far from the origin -------------------------------------------------------------------
def test_tight_cluster(pkg):
    k, m, n = 32, 64, 4000
    r = (np.float32(1000) + np.float32(1e-4) * _rand(71, n, k)).astype(np.float32)
    q = (np.float32(1000) + np.float32(1e-4) * _rand(72, m, k)).astype(np.float32)
    d = v0_all(q, r)
    radius2 = float(np.median(d))
    ix = pkg.Index(_dev(r), range_mfma=True)
    got, info = _search(ix, _dev(q), radius2)
    _assert_same(got, range_oracle(q, r, radius2), "cluster")
    assert info["path"] == MFMA                          # (the filter may flag everything here)
    ix.close()


# ---- 7. underflow and large scale -----------------------------------------------------------------------------
@pytest.mark.parametrize("exp", [-70, 20])
def test_scaled_data(pkg, exp):
    k, m, n = 16, 130, 2999
    s = np.float32(2.0 ** exp)
    q = _rand(10 + k, m, k) * s                          # test 1's data, re-scaled exactly
    r = _rand(20 + k, n, k) * s
    r[100:140] = r[7]
    radii = _radii(v0_all(q, r), n)[:3]
    ix = pkg.Index(_dev(r), range_mfma=True)
    qd = _dev(q)
    for radius2 in radii:
        got, info = _search(ix, qd, radius2)
        _assert_same(got, range_oracle(q, r, radius2), f"scale 2^{exp} r2={radius2}")
        assert info["path"] == MFMA
    ix.close()


# ---- 8. non-finite values -------------------------------------------------------------------------------------
def test_nonfinite_queries_refs_and_few_queries(pkg):
    k, m, n = 16, 72, 4000
    q = _rand(81, m, k)
    r = _rand(82, n, k)
    q[5, 3] = np.nan
    q[40, 0] = 1e20
    radius2 = _radii(v0_all(q[:5], r), n)[1]              # about 3 hits per query
    want = range_oracle(q, r, radius2)
    assert want[0][6] == want[0][5] and want[0][41] == want[0][40]       # V0: those rows hit nothing
    ix = pkg.Index(_dev(r), range_mfma=True)
    got, info = _search(ix, _dev(q), radius2)
    _assert_same(got, want, "void queries")
    nblk = -(-n // 32)
    assert info["path"] == MFMA and 2 * nblk <= info["flagged"] <= 2 * nblk + 20 * m   # two filled rows; the rest filtered
    got, info = _search(ix, _dev(q[:10]), radius2)       # below the filter's query floor
    _assert_same(got, range_oracle(q[:10], r, radius2), "few queries")
    assert info["path"] == EXACT
    ix.close()
    r[77, 2] = np.inf                                    # refs_bad
    q = _rand(83, m, k)
    ix = pkg.Index(_dev(r), range_mfma=True)
    got, info = _search(ix, _dev(q), radius2)
    _assert_same(got, range_oracle(q, r, radius2), "inf ref")
    assert info["path"] == EXACT and ix.stats()["path"] == EXACT
    ix.close()


# ---- 9. index options -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["auto", "exact", "mfma"])
def test_index_options(pkg, path):
    k, m, n = 32, 70, 5000
    q = _rand(91, m, k)
    r = _rand(92, n, k)
    radius2 = _radii(v0_all(q, r), n)[2]
    base = 10 ** 6
    want = range_oracle(q, r, radius2, index_base=base)
    qd = _dev(q)
    ix = pkg.Index(_dev(r), path=path, index_base=base, range_mfma=True)
    got, info = _search(ix, qd, radius2)
    _assert_same(got, want, f"path={path}")
    assert info["path"] == MFMA
    if path == "exact":
        ref = pkg.Index(_dev(r), path="exact", index_base=base)
        assert torch.equal(ix.search_keys(qd), ref.search_keys(qd))
        assert ix.stats()["path"] == EXACT
        ref.close()
    ix.close()
    soa = pkg.Index(_dev(np.ascontiguousarray(r.T)), path=path, index_base=base, soa=True, range_mfma=True)
    got, info = _search(soa, qd, radius2)
    _assert_same(got, want, f"soa path={path}")
    assert info["path"] == MFMA
    soa.close()


# ---- 10. the count / fill contract ----------------------------------------------------------------------------
def test_count_fill_contract(pkg):
    k, m, n = 16, 80, 30000
    q = _rand(111, m, k)
    r = _rand(112, n, k)
    radius2 = _radii(v0_all(q, r), n)[2]
    want = range_oracle(q, r, radius2)
    qd, rd = _dev(q), _dev(r)
    q2 = _dev(_rand(113, 300, k))
    L = pkg.lib
    ix = pkg.Index(rd, path="mfma", range_mfma=True)
    ref_keys = ix.search_keys(q2).clone()
    ref_topk = ix.search_topk_keys(q2, 7).clone()
    lims = ix.range_count(qd, radius2)
    assert ix.range_info()["path"] == MFMA
    total = int(lims[-1].item())
    idx = torch.full((total,), -7, dtype=torch.int32, device=DEV)
    dist = torch.full((total,), -1.0, dtype=torch.float32, device=DEV)
    args = (lims.data_ptr(), idx.data_ptr(), dist.data_ptr(), None)
    assert L.nns_index_range_fill(ix._h, m, qd.data_ptr(), float(np.float32(radius2) * np.float32(2)), *args) == 1
    assert L.nns_index_range_fill(ix._h, m - 1, qd.data_ptr(), radius2, *args) == 1
    keys = ix.search_keys(q2)                            # a 1-NN (through the filter: it prepares ITS queries in the
    tk = ix.search_topk_keys(q2, 7)                      # shared workspaces) and a top-K search in between
    ix.range_fill(qd, radius2, lims, idx=idx, dist=dist, return_distances=True)
    _assert_same(_host((lims, idx, dist)), want, "interleaved")
    assert torch.equal(keys, ref_keys) and torch.equal(tk, ref_topk)
    ix.close()
    # no hits: null idx / dist
    far = _dev(_rand(114, m, k) + np.float32(10))
    ix = pkg.Index(rd, range_mfma=True)
    lims = ix.range_count(far, 1.0)
    info = ix.range_info()
    assert info["path"] == MFMA and info["flagged"] == 0 and info["hits"] == 0
    assert L.nns_index_range_fill(ix._h, m, far.data_ptr(), 1.0, lims.data_ptr(), None, None, None) == 0
    torch.cuda.synchronize()
    assert not torch.any(lims)
    ix.close()


# ---- 11. determinism ------------------------------------------------------------------------------------------
def test_deterministic_buffers(pkg):
    k, m, n = 16, 256, 50000
    qd = torch.empty((m, k), dtype=torch.float32, device=DEV)
    rd = torch.empty((n, k), dtype=torch.float32, device=DEV)
    pkg.fill_uniform(qd, 5, 0)
    pkg.fill_uniform(rd, 6, 0)
    ix = pkg.Index(rd, range_mfma=True)
    runs = []
    for garbage in (-7, 0x5A5A5A5A):
        lims = torch.full((m + 1,), garbage, dtype=torch.int64, device=DEV)
        ix.range_count(qd, 0.45, lims=lims)
        info = ix.range_info()
        total = int(lims[-1].item())
        idx = torch.full((total,), garbage, dtype=torch.int32, device=DEV)
        dist = torch.full((total,), float(garbage), dtype=torch.float32, device=DEV)
        ix.range_fill(qd, 0.45, lims, idx=idx, dist=dist, return_distances=True)
        runs.append((_host((lims, idx, dist)), info))
    (a, ia), (b, ib) = runs
    assert ia == ib and ia["path"] == MFMA and ia["hits"] > m
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    sel = [0, 1, 100, 255]
    want = range_oracle(qd.cpu().numpy()[sel], rd.cpu().numpy(), 0.45)
    lims, idx, dist = a
    got_i = np.concatenate([idx[lims[i]:lims[i + 1]] for i in sel])
    got_d = np.concatenate([dist[lims[i]:lims[i + 1]] for i in sel])
    got_l = np.concatenate([[0], np.cumsum([lims[i + 1] - lims[i] for i in sel])])
    _assert_same((got_l, got_i, got_d), want, "determinism sample")
    ix.close()


# ---- 12. query batches ----------------------------------------------------------------------------------------
def test_two_query_batches(pkg):
    """2^20 queries x 70000 refs at k = 8 need 69 flag words per query: two batches under the 256 MiB cap.  The whole
    result equals K7's on an unflagged index (itself held against the oracle by test_range_gpu.py); queries around
    the batch boundary and at both ends are held against the oracle directly."""
    k, m, n = 8, 1 << 20, 70000
    p = pkg.plan_range_mfma(k, m, n)
    assert p["batches"] == 2
    qd = torch.empty((m, k), dtype=torch.float32, device=DEV)
    rd = torch.empty((n, k), dtype=torch.float32, device=DEV)
    pkg.fill_uniform(qd, 15, 0)
    pkg.fill_uniform(rd, 16, 0)
    radius2 = 0.05                                       # about one hit per query
    ix = pkg.Index(rd, range_mfma=True)
    got = ix.search_range(qd, radius2, return_distances=True)
    info = ix.range_info()
    assert info["path"] == MFMA and info["hits"] == int(got[0][-1].item()) > m // 8
    ref = pkg.Index(rd)
    want = ref.search_range(qd, radius2, return_distances=True)
    assert ref.range_info()["path"] == EXACT
    torch.cuda.synchronize()
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    b = p["batch"]
    sel = [0, 1, b - 2, b - 1, b, b + 1, m - 2, m - 1]
    lims = got[0].cpu().numpy()
    idx, dist = got[1].cpu().numpy(), got[2].cpu().numpy()
    worc = range_oracle(qd[sel].cpu().numpy(), rd.cpu().numpy(), radius2)
    got_i = np.concatenate([idx[lims[i]:lims[i + 1]] for i in sel])
    got_d = np.concatenate([dist[lims[i]:lims[i + 1]] for i in sel])
    got_l = np.concatenate([[0], np.cumsum([lims[i + 1] - lims[i] for i in sel])])
    _assert_same((got_l, got_i, got_d), worc, "batch boundary")
    ix.close()
    ref.close()


# ---- 13. the caller's stream and device -----------------------------------------------------------------------
def test_caller_stream_and_device_restored(pkg):
    k, m, n = 16, 70, 8000
    q = _rand(101, m, k)
    r = _rand(102, n, k)
    radius2 = _radii(v0_all(q, r), n)[2]
    want = range_oracle(q, r, radius2)
    dev_before = torch.cuda.current_device()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        qd = torch.from_numpy(q).to(DEV)
        rd = torch.from_numpy(r).to(DEV)
    s.synchronize()
    ix = pkg.Index(rd, stream=s, range_mfma=True)
    lims, idx, dist = ix.search_range(qd, radius2, return_distances=True, stream=s)
    s.synchronize()
    _assert_same((lims.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy()), want, "caller stream")
    assert ix.range_info()["path"] == MFMA
    ix.close()
    _assert_same(pkg.search_range(q, r, radius2, return_distances=True, range_mfma=True), want, "whole")
    assert torch.cuda.current_device() == dev_before


# ---- 14. every pass kind of a profiled index ends in the same bookkeeping -------------------------------------
STAGES = ("prep_queries_ms", "filter_ms", "finalize_ms", "rerank_ms", "exact_ms")


def _check_stats(ix, path, what):
    """nns_index_stats after one pass: the reported path, every time finite and >= 0, the stages of the pass's path
    (and only those) within the total.  The stages are consecutive sub-intervals of the total between the same
    events, so their sum can pass it only by the fp32 roundings of the five elapsed times (2^-24 relative each):
    1e-5 relative + 1e-6 ms covers them."""
    st = ix.stats()
    assert st["path"] == path, (what, st)
    for name in STAGES + ("prep_refs_ms", "total_ms"):
        assert np.isfinite(st[name]) and st[name] >= 0.0, (what, name, st)
    assert st["total_ms"] > 0.0, (what, st)
    assert sum(st[s] for s in STAGES) <= st["total_ms"] * (1 + 1e-5) + 1e-6, (what, st)
    if path == MFMA:
        assert st["exact_ms"] == 0.0, (what, st)
    else:
        assert all(st[s] == 0.0 for s in STAGES[:4]), (what, st)
    return st


def test_profiled_index_after_every_pass_kind(pkg):
    """nns_index_stats and nns_index_range_info after each pass kind on NNS_PROFILE indices: exact 1-NN, MFMA 1-NN,
    top-K, range count and fill on the exact path (below the filtered path's 64-query floor) and on the filtered path.
    Expected answers: the V0 oracle, and an exact-path index without either flag.  (nns_stats does not export the
    query count of the last pass; the filtered count's examined pairs, m x blocks, show it.)"""
    k, m, n, kn, few = 16, 128, 4096, 8, 32
    qd = torch.empty((m, k), dtype=torch.float32, device=DEV)
    rd = torch.empty((n, k), dtype=torch.float32, device=DEV)
    pkg.fill_uniform(qd, 31)
    pkg.fill_uniform(rd, 32)
    torch.cuda.synchronize()
    q, r = qd.cpu().numpy(), rd.cpu().numpy()
    d = v0_all(q, r)
    order = np.argsort(d, axis=1, kind="stable")                 # (distance, index) order: V0's tie rule
    radius2 = float(np.median(np.take_along_axis(d, order[:, 9:10], axis=1)))   # about ten hits per query
    want_range = range_oracle(q, r, radius2)
    want_few = range_oracle(q[:few], r, radius2)
    assert 5 * m < want_range[0][-1] < 20 * m
    want_nn = (order[:, 0].astype(np.int32), np.take_along_axis(d, order[:, :1], axis=1)[:, 0])
    want_topk = (order[:, :kn].astype(np.int32), np.take_along_axis(d, order[:, :kn], axis=1))
    qfew = qd[:few].contiguous()

    # the exact-path index: the oracle's answers
    ref = pkg.Index(rd, path="exact")
    ref_nn = _host(ref.search(qd, return_distances=True))
    ref_topk = _host(ref.search_topk(qd, kn, return_distances=True))
    ref_range = _host(ref.search_range(qd, radius2, return_distances=True))
    ref_few = _host(ref.search_range(qfew, radius2, return_distances=True))
    ref.close()
    for got, want in ((ref_nn, want_nn), (ref_topk, want_topk)):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    _assert_same(ref_range, want_range, "exact index")
    _assert_same(ref_few, want_few, "exact index, few queries")

    def same(got, ref_out, what):                                # (distances by their bits)
        for a, b in zip(got, ref_out):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what

    # exact 1-NN
    ex = pkg.Index(rd, path="exact", profile=True, range_mfma=True)
    same(_host(ex.search(qd, return_distances=True)), ref_nn, "exact 1-NN")
    _check_stats(ex, EXACT, "exact 1-NN")
    ex.close()

    ix = pkg.Index(rd, path="mfma", profile=True, range_mfma=True)
    # MFMA 1-NN
    same(_host(ix.search(qd, return_distances=True)), ref_nn, "MFMA 1-NN")
    st = _check_stats(ix, MFMA, "MFMA 1-NN")
    assert st["k_tile"] == 16 and st["filter_ms"] > 0.0, st
    # top-K: an exact pass of the MFMA index
    same(_host(ix.search_topk(qd, kn, return_distances=True)), ref_topk, "top-K")
    assert _check_stats(ix, EXACT, "top-K")["exact_ms"] > 0.0
    # range count and fill, exact path (fewer than 64 queries) and filtered path
    blocks = pkg.plan_range_mfma(k, m, n)["blocks_per_query"]
    for what, queries, mm, path, want, ref_out in (("exact range", qfew, few, EXACT, want_few, ref_few),
                                                   ("filtered range", qd, m, MFMA, want_range, ref_range)):
        lims = ix.range_count(queries, radius2)
        _check_stats(ix, path, what + " count")
        info = ix.range_info()
        total = int(lims[-1].item())
        assert info["path"] == path and info["hits"] == total == want[0][-1], (what, info, total)
        assert info["examined"] == (mm * blocks if path == MFMA else 0), (what, info)
        if path == MFMA:
            assert 0 < info["flagged"] <= info["examined"], (what, info)
        idx, dist = ix.range_fill(queries, radius2, lims, total=total, return_distances=True)
        _check_stats(ix, path, what + " fill")
        assert ix.range_info() == info, what                     # the fill leaves the count's record
        got = _host((lims, idx, dist))
        _assert_same(got, want, what)
        same(got, ref_out, what)
    ix.close()
