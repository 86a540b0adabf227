"""GPU tests of the MFMA-filtered range search for bf16 points (NNS_RANGE_MFMA on a bf16 index: the 16x16x32 flag kernel
over the order-1 image, 32 <= k <= 256).  Lims, indices and distance bits equal the numpy range oracle of
test_range_cpu.py on the bf16 values widened to fp32, through the split API of a flagged index and the whole call — a
grid over k, several ring slots / splits / chunks and block edges, the inclusive boundary, bounds on the number of
flagged blocks from the mode-1 threshold's model, re-scaled data, non-finite queries and refs, the split-API contract
and query batches."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_range_cpu import range_oracle, v0_all  # noqa: E402
from test_range_gpu import _as_searched, _assert_same, _radii, _to_dev  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
INF = float("inf")
EXACT, MFMA = 1, 2


def _rand(seed, *shape):
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


def _pts(pkg, seed, *shape):
    """uniform [0, 1) values rounded to bf16, as fp32"""
    return _as_searched(pkg, _rand(seed, *shape), True)


def _dev(pkg, a):
    return _to_dev(pkg, a, True)


def _host(out):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _search(ix, qd, radius2):
    """((lims, idx, dist) on the host, range_info of the count) of one split-API range search."""
    out = ix.search_range(qd, radius2, return_distances=True)
    return _host(out), ix.range_info()


def _whole(pkg, q, r, radius2):
    return pkg.search_range_bf16(pkg.to_bf16_bits(q), pkg.to_bf16_bits(r), radius2, return_distances=True, range_mfma=True)


# ---- (a) a grid over k: both depths, k below / at / above a whole tile -------------------------------------------
@pytest.mark.parametrize("k", [32, 40, 64, 100, 128, 129, 200, 256])
def test_grid(pkg, k):
    m, n = 130, 2999
    q = _pts(pkg, 10 + k, m, k)
    r = _pts(pkg, 20 + k, n, k)
    r[100:140] = r[7]                                    # a run of equal distances for every query
    radii = _radii(v0_all(q, r), n)
    blocks = pkg.plan_range_mfma(k, m, n, bf16=True)["blocks_per_query"]
    ix = pkg.Index(_dev(pkg, r), range_mfma=True)
    qd = _dev(pkg, q)
    for radius2 in radii:
        want = range_oracle(q, r, radius2)
        got, info = _search(ix, qd, radius2)
        _assert_same(got, want, f"split k={k} r2={radius2}")
        assert info["path"] == (EXACT if radius2 == INF else MFMA), (radius2, info)   # +INF takes K7
        assert info["hits"] == want[0][-1]
        if radius2 != INF:
            assert info["examined"] == m * blocks
            assert ix.stats()["path"] == MFMA
        _assert_same(_whole(pkg, q, r, radius2), want, f"whole k={k} r2={radius2}")
    ix.close()


# ---- (b) several ring slots, splits and chunks; block edges -------------------------------------------------------
def test_slots_splits_chunks_and_block_edges(pkg):
    k, m, n = 32, 600, 70001                             # two query groups of 512; 69 flag words: two chunks
    p = pkg.plan_range_mfma(k, m, n, bf16=True)
    assert p["grid_x"] == 2 and p["grid_y"] > 1
    assert -(-p["blocks_per_query"] // 32) == 69
    assert pkg.plan_topk_mfma(k, m, n, 1, bf16=True)["chunks"] == 2          # (the evaluation's chunks are the selection's)
    q = _pts(pkg, 41, m, k)
    r = _pts(pkg, 42, n, k)
    spots = (0, 31, 32, n - 1, n - 9, 2047 * 32 + 5, 2048 * 32)
    for i, j in enumerate(spots):
        r[j] = q[7 * i]                                  # exact duplicates at block edges, chunk edge, last block
    d = v0_all(q, r)
    radius2 = _radii(d, n)[1]                            # about 3 hits per query
    want = range_oracle(q, r, radius2)
    assert 2 * m < want[0][-1] < 6 * m
    ix = pkg.Index(_dev(pkg, r), range_mfma=True)
    got, info = _search(ix, _dev(pkg, q), radius2)
    _assert_same(got, want, "edges")
    assert info["path"] == MFMA and 0 < info["flagged"] < info["examined"] // 4
    for i, j in enumerate(spots):
        row = slice(got[0][7 * i], got[0][7 * i + 1])
        assert j in got[1][row].tolist() and got[2][row][got[1][row] == j] == 0.0, (i, j)
    _assert_same(_whole(pkg, q, r, radius2), want, "whole edges")
    ix.close()


# ---- (c) the inclusive boundary -----------------------------------------------------------------------------------
def test_radius_is_inclusive_and_next_float_excluded(pkg):
    k, m, n = 40, 64, 5000
    q = _pts(pkg, 51, m, k)
    r = _pts(pkg, 52, n, k)
    d = v0_all(q, r)
    ix = pkg.Index(_dev(pkg, r), range_mfma=True)
    qd = _dev(pkg, q)
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


# ---- (d) the number of flagged blocks lies between the model's bounds ----------------------------------------------
def test_flag_bounds(pkg):
    """Every block holding a hit is flagged, and a flagged block holds a ref with
    d <= radius2 + 2 tau_1(radius2 - |x|^2) + 2^-21 (radius2 + |x|^2): the threshold is a + 1.002 tau_1(a) + 2^-22 (radius2
    + |x|^2) and a score lies within tau_1 / 2 of d - |x|^2 (DESIGN section 4, K7m, bf16 points).  Norms are the
    uncentred ones, recomputed in fp64; 1e-5 relative on the upper radius covers their rounding to fp32.  (On this
    data: lo = 1263, hi = 1280 of 80000 pairs, and both a numpy restatement of the scores and the kernel flag 1269.)"""
    k, m, n = 64, 128, 20000
    q = _pts(pkg, 61, m, k)
    r = _pts(pkg, 62, n, k)
    d = v0_all(q, r)
    radius2 = float(np.sort(d.ravel())[10 * m])          # about 10 hits per query
    kt = pkg.plan_range_mfma(k, m, n, bf16=True)["kt"]
    qn = (q.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
    ymax2 = float((r.astype(np.float64) ** 2).sum(axis=1).max().astype(np.float32))
    nblk = -(-n // 32)
    dpad = np.full((m, nblk * 32), np.inf, np.float32)
    dpad[:, :n] = d
    bmin = dpad.reshape(m, nblk, 32).min(axis=2)         # the nearest ref of every (query, block)
    lo = int((bmin <= np.float32(radius2)).sum())
    hi = 0
    for i in range(m):
        c0, c1, x2 = pkg.tau_consts(kt, float(qn[i]), ymax2, 1)
        tau = c0 + c1 * max(radius2 - float(qn[i]) + x2, 0.0)
        upper = (radius2 + 2.0 * tau + 2.0 ** -21 * (radius2 + float(qn[i]))) * (1.0 + 1e-5)
        hi += int((bmin[i].astype(np.float64) <= upper).sum())
    ix = pkg.Index(_dev(pkg, r), range_mfma=True)
    got, info = _search(ix, _dev(pkg, q), radius2)
    _assert_same(got, range_oracle(q, r, radius2), "flag bounds")
    print(f"flagged {info['flagged']} of {info['examined']} (lo {lo}, hi {hi})")
    assert info["path"] == MFMA
    assert info["examined"] == m * pkg.plan_range_mfma(k, m, n, bf16=True)["blocks_per_query"]
    assert lo <= info["flagged"] <= hi, (lo, info, hi)
    assert hi < m * nblk // 2                            # (the bound says something: far from "everything")
    ix.close()


# ---- (e) underflow and large scale (a power of two is exact in bf16) ------------------------------------------------
@pytest.mark.parametrize("exp", [-70, 20])
def test_scaled_data(pkg, exp):
    k, m, n = 32, 130, 2999
    s = np.float32(2.0 ** exp)
    q = _pts(pkg, 10 + k, m, k) * s                      # test (a)'s data, re-scaled exactly
    r = _pts(pkg, 20 + k, n, k) * s
    r[100:140] = r[7]
    assert np.array_equal(q, _as_searched(pkg, q, True)) and np.array_equal(r, _as_searched(pkg, r, True))
    radii = _radii(v0_all(q, r), n)[:3]
    ix = pkg.Index(_dev(pkg, r), range_mfma=True)
    qd = _dev(pkg, q)
    for radius2 in radii:
        got, info = _search(ix, qd, radius2)
        _assert_same(got, range_oracle(q, r, radius2), f"scale 2^{exp} r2={radius2}")
        assert info["path"] == MFMA
    ix.close()


# ---- (f) non-finite and huge values, too few queries ---------------------------------------------------------------
def test_nonfinite_queries_refs_and_few_queries(pkg):
    k, m, n = 32, 72, 4000
    q = _pts(pkg, 81, m, k)
    r = _pts(pkg, 82, n, k)
    radius2 = _radii(v0_all(q, r), n)[1]                 # about 3 hits per query
    q[5, 3] = np.nan
    q[17, 31] = np.inf
    q[40, 0] = _as_searched(pkg, np.float32([1e18]), True)[0]
    want = range_oracle(q, r, radius2)
    for i in (5, 17, 40):
        assert want[0][i + 1] == want[0][i]              # V0: those rows hit nothing
    ix = pkg.Index(_dev(pkg, r), range_mfma=True)
    got, info = _search(ix, _dev(pkg, q), radius2)
    _assert_same(got, want, "void queries")
    nblk = -(-n // 32)
    assert info["path"] == MFMA and 3 * nblk <= info["flagged"] <= 3 * nblk + 20 * m   # three filled rows; the rest filtered
    got, info = _search(ix, _dev(pkg, q[:63]), radius2)  # below the filter's query floor
    _assert_same(got, range_oracle(q[:63], r, radius2), "63 queries")
    assert info["path"] == EXACT
    ix.close()
    q = _pts(pkg, 83, m, k)
    for bad in (np.nan, np.inf, _as_searched(pkg, np.float32([1e18]), True)[0]):
        rb = r.copy()
        rb[77, 2] = bad                                  # refs_bad
        ix = pkg.Index(_dev(pkg, rb), range_mfma=True)
        got, info = _search(ix, _dev(pkg, q), radius2)
        _assert_same(got, range_oracle(q, rb, radius2), f"ref holding {bad}")
        assert info["path"] == EXACT and ix.stats()["path"] == EXACT
        ix.close()


# ---- (g) the split-API contract ------------------------------------------------------------------------------------
def test_index_base_soa_and_refresh(pkg):
    k, m, n = 48, 70, 5000
    q = _pts(pkg, 91, m, k)
    r = _pts(pkg, 92, n, k)
    radius2 = _radii(v0_all(q, r), n)[2]
    base = 10 ** 6
    want = range_oracle(q, r, radius2, index_base=base)
    qd = _dev(pkg, q)
    for path in ("auto", "exact"):
        ix = pkg.Index(_dev(pkg, r), path=path, index_base=base, range_mfma=True)
        got, info = _search(ix, qd, radius2)
        _assert_same(got, want, f"path={path}")
        assert info["path"] == MFMA
        ix.close()
    soa = pkg.Index(_dev(pkg, np.ascontiguousarray(r.T)), index_base=base, soa=True, range_mfma=True)
    got, info = _search(soa, qd, radius2)
    _assert_same(got, want, "soa")
    assert info["path"] == MFMA
    soa.close()
    rd = _dev(pkg, r)
    ix = pkg.Index(rd, range_mfma=True)
    r2 = _pts(pkg, 93, n, k)
    rd.copy_(_dev(pkg, r2))                              # rewritten in place
    ix.refresh()
    got, info = _search(ix, qd, radius2)
    _assert_same(got, range_oracle(q, r2, radius2), "refreshed")
    assert info["path"] == MFMA
    r2[5, 5] = np.inf
    rd.copy_(_dev(pkg, r2))
    ix.refresh()
    got, info = _search(ix, qd, radius2)                 # the refresh is looked at before the filtered path is taken
    _assert_same(got, range_oracle(q, r2, radius2), "refreshed, inf ref")
    assert info["path"] == EXACT
    ix.close()


def test_count_fill_contract_determinism_and_stream(pkg):
    k, m, n = 32, 80, 30000
    q = _pts(pkg, 111, m, k)
    r = _pts(pkg, 112, n, k)
    radius2 = _radii(v0_all(q, r), n)[2]
    want = range_oracle(q, r, radius2)
    dev_before = torch.cuda.current_device()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        qd, rd = _dev(pkg, q), _dev(pkg, r)
        q2 = _dev(pkg, _pts(pkg, 113, 300, k))
    s.synchronize()
    L = pkg.lib
    ix = pkg.Index(rd, path="mfma", stream=s, range_mfma=True)
    with torch.cuda.stream(s):                           # (the copy on the stream the search ran on)
        ref_keys = ix.search_keys(q2, stream=s).clone()
    s.synchronize()
    runs = []
    for garbage in (-7, 0x5A5A5A5A):
        with torch.cuda.stream(s):                       # (the buffers are filled on the stream the passes run on)
            lims = torch.full((m + 1,), garbage, dtype=torch.int64, device=DEV)
            ix.range_count(qd, radius2, lims=lims, stream=s)
            info = ix.range_info()
            assert info["path"] == MFMA
            total = int(lims[-1].item())
            idx = torch.full((total,), garbage, dtype=torch.int32, device=DEV)
            dist = torch.full((total,), float(garbage), dtype=torch.float32, device=DEV)
            args = (lims.data_ptr(), idx.data_ptr(), dist.data_ptr(), s.cuda_stream)
            assert L.nns_index_range_fill(ix._h, m, qd.data_ptr(), float(np.float32(radius2) * np.float32(2)), *args) == 1
            assert L.nns_index_range_fill(ix._h, m - 1, qd.data_ptr(), radius2, *args) == 1
            keys = ix.search_keys(q2, stream=s)          # a 1-NN search through the bf16 filter in between: it prepares
            ix.range_fill(qd, radius2, lims, idx=idx, dist=dist, return_distances=True, stream=s)   # ITS queries
            s.synchronize()
            assert torch.equal(keys, ref_keys)
        runs.append((_host((lims, idx, dist)), info))
    (a, ia), (b, ib) = runs
    _assert_same(a, want, "interleaved, caller stream")
    assert ia == ib and ia["hits"] == want[0][-1]
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    ix.close()
    assert torch.cuda.current_device() == dev_before


# ---- (h) query batches ---------------------------------------------------------------------------------------------
def test_two_query_batches(pkg):
    """4096 queries x (2^24 + 1) refs at k = 32 need 16385 flag words per query: two batches under the 256 MiB cap (the
    fp32 test's 2^36 pairs, with the factor on the refs).  The whole result equals K7's on an unflagged index (itself
    held against the oracle by test_range_gpu.py); queries at the batch boundary and at both ends are held against
    the oracle directly.  The radius is read off the exact 1-NN distances of a few queries: about one hit per query."""
    k, m, n = 32, 4096, (1 << 24) + 1
    p = pkg.plan_range_mfma(k, m, n, bf16=True)
    assert p["batches"] == 2
    g = torch.Generator(device=DEV)
    g.manual_seed(15)
    qd = torch.rand((m, k), generator=g, device=DEV).to(torch.bfloat16)
    rd = torch.empty((n, k), dtype=torch.bfloat16, device=DEV)
    for c0 in range(0, n, 1 << 22):
        c1 = min(n, c0 + (1 << 22))
        rd[c0:c1] = torch.rand((c1 - c0, k), generator=g, device=DEV).to(torch.bfloat16)
    ref = pkg.Index(rd, path="exact")
    _, d1 = ref.search(qd[:256].contiguous(), return_distances=True)
    radius2 = float(d1.median().item())
    ix = pkg.Index(rd, path="exact", range_mfma=True)
    got = ix.search_range(qd, radius2, return_distances=True)
    info = ix.range_info()
    assert info["path"] == MFMA and info["hits"] == int(got[0][-1].item()) > m // 8
    assert info["examined"] == m * p["blocks_per_query"] and 0 < info["flagged"] < info["examined"] // 4
    want = ref.search_range(qd, radius2, return_distances=True)
    assert ref.range_info()["path"] == EXACT
    torch.cuda.synchronize()
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    b = p["batch"]
    sel = [0, b - 1, b, m - 1]
    lims = got[0].cpu().numpy()
    idx, dist = got[1].cpu().numpy(), got[2].cpu().numpy()
    qs = qd[sel].float().cpu().numpy()
    counts = np.zeros(len(sel), np.int64)
    rows = [([], []) for _ in sel]
    for c0 in range(0, n, 1 << 22):                      # the oracle over ref chunks: ascending index within a query
        rc = rd[c0:c0 + (1 << 22)].float().cpu().numpy()
        wl, wi, wd = range_oracle(qs, rc, radius2, index_base=c0)
        for t in range(len(sel)):
            rows[t][0].append(wi[wl[t]:wl[t + 1]])
            rows[t][1].append(wd[wl[t]:wl[t + 1]])
            counts[t] += wl[t + 1] - wl[t]
    worc = (np.concatenate([[0], np.cumsum(counts)]), np.concatenate([np.concatenate(x[0]) for x in rows]),
            np.concatenate([np.concatenate(x[1]) for x in rows]))
    got_i = np.concatenate([idx[lims[i]:lims[i + 1]] for i in sel])
    got_d = np.concatenate([dist[lims[i]:lims[i + 1]] for i in sel])
    got_l = np.concatenate([[0], np.cumsum([lims[i + 1] - lims[i] for i in sel])])
    _assert_same((got_l, got_i, got_d), worc, "batch boundary")
    ix.close()
    ref.close()
