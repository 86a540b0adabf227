"""GPU tests of the range search (fixed-radius neighbours, K7) against the numpy range oracle of test_range_cpu.py:
lims and indices exact, distances bit for bit, on the whole-call and split APIs — a random grid over k and both point
types, every scan instantiation, ties at the radius and across chunk boundaries, non-finite data, cross-checks with
top-K, index paths and SoA refs, index_base, streams, the count / fill contract, shards, a total above 2^31 and
statistics."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_range_cpu import RANGE_CASES, range_case_id, range_oracle, scan_vec, v0_all  # noqa: E402
from test_topk_edges_gpu import _as_searched, _to_dev  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
INF = float("inf")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rand(seed, *shape):
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


def _assert_same(got, want, what):
    lims, idx, dist = (np.asarray(a) for a in got)
    wl, wi, wd = want
    assert np.array_equal(lims, wl), f"{what}: lims differ (first at {np.argmax(lims != wl) if lims.shape == wl.shape else 'shape'})"
    bad = np.argwhere(idx != wi)
    assert bad.size == 0, f"{what}: {len(bad)} index mismatches, first at {bad[:3].ravel().tolist()}"
    assert np.array_equal(_bits(dist), _bits(wd)), f"{what}: distance bits differ"


def _whole(pkg, q, r, radius2, bf16=False, **kw):
    """The whole call on the searched values (bf16: the rounded bit patterns) with distances."""
    if bf16:
        return pkg.search_range_bf16(pkg.to_bf16_bits(q), pkg.to_bf16_bits(r), radius2, return_distances=True, **kw)
    return pkg.search_range(q, r, radius2, return_distances=True, **kw)


def _index_range(pkg, refs, queries, radius2, **kw):
    """(lims, idx, dist) of one Index.search_range (host arrays)."""
    ix = pkg.Index(refs, **kw)
    lims, idx, dist = ix.search_range(queries, radius2, return_distances=True)
    torch.cuda.synchronize()
    ix.close()
    return lims.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy()


def _radii(d, n):
    """Squared radii for about 0, a few, thousands and all hits per query (values the distances take, so that the
    inclusive compare is exercised)."""
    fin = np.sort(d[np.isfinite(d)].ravel())
    pick = lambda frac: float(fin[min(len(fin) - 1, int(frac * len(fin)))])  # noqa: E731
    zero = float(np.nextafter(fin[0], np.float32(0))) if fin[0] > 0 else 0.0
    return [zero, pick(3.0 / n), pick(min(0.9, 2000.0 / n)), INF]


# ---- 1. a random grid over k and both point types --------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("k", [1, 3, 16, 33, 128, 1000, 4096, 16384])
def test_random_grid(pkg, k, bf16):
    m, n = (37, 2999) if k <= 1000 else (11, 1999)      # m not a multiple of the tile, n not of 256
    q = _as_searched(pkg, _rand(10 + k, m, k), bf16)
    r = _as_searched(pkg, _rand(20 + k, n, k), bf16)
    r[100:140] = r[7]                                    # a run of equal distances for every query
    d = v0_all(q, r)
    for radius2 in _radii(d, n):
        want = range_oracle(q, r, radius2)
        _assert_same(_whole(pkg, q, r, radius2, bf16), want, f"whole k={k} bf16={bf16} r2={radius2}")
    radius2 = _radii(d, n)[2]
    got = _index_range(pkg, _to_dev(pkg, r, bf16), _to_dev(pkg, q, bf16), radius2, path="exact")
    _assert_same(got, range_oracle(q, r, radius2), f"split k={k} bf16={bf16}")


# ---- 2. every scan instantiation -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RANGE_CASES, ids=[range_case_id(c) for c in RANGE_CASES])
def test_every_range_instantiation(pkg, case):
    bf16 = case.dtype == "bf16"
    k, m, n = case.k, case.m, case.n
    assert pkg.plan_range(k, m, n, bf16=bf16)["queries_per_wg"] == case.qt
    seed = 7 * k + 131 * m
    q = _as_searched(pkg, _rand(seed, m, k) * np.float32(2) - np.float32(1), bf16)
    r = _as_searched(pkg, _rand(seed + 1, n, k) * np.float32(2) - np.float32(1), bf16)
    r[n // 2:n // 2 + 40] = r[3]
    radius2 = _radii(v0_all(q, r), n)[2]
    want = range_oracle(q, r, radius2)
    esz = 2 if bf16 else 4
    flat = _to_dev(pkg, r, bf16).reshape(-1)
    buf = torch.empty(case.offset + n * k, dtype=flat.dtype, device=DEV)
    buf[case.offset:].copy_(flat)
    view = buf[case.offset:].view(n, k)                  # storage offset: the pointer may be misaligned on purpose
    assert scan_vec(k, view.data_ptr(), esz) == case.vec
    runs = [view]
    if case.vec == 1 and k % 4 == 0:
        aligned = view.clone()                           # the same data through the 4-wide loads
        assert scan_vec(k, aligned.data_ptr(), esz) == 4
        runs.append(aligned)
    qd = _to_dev(pkg, q, bf16)
    for refs in runs:
        got = _index_range(pkg, refs, qd, radius2, path="exact")
        _assert_same(got, want, f"{range_case_id(case)} VEC={scan_vec(k, refs.data_ptr(), esz)}")
    _assert_same(_whole(pkg, q, r, radius2, bf16), want, f"{range_case_id(case)} whole")


# ---- 3. boundary ties -------------------------------------------------------------------------------------------
def test_radius_is_inclusive_and_next_float_excluded(pkg):
    k, m, n = 3, 20, 5000
    q = _rand(31, m, k)
    r = _rand(32, n, k)
    d = v0_all(q, r)
    for i in (0, 7, 19):
        j = int(np.argsort(d[i])[50])
        radius2 = float(d[i, j])
        at = pkg.search_range(q[i:i + 1], r, radius2, return_distances=True)
        assert j in at[1].tolist()                                   # at exactly radius2: in
        below = float(np.nextafter(np.float32(radius2), np.float32(0)))
        short = pkg.search_range(q[i:i + 1], r, below, return_distances=True)
        assert j not in short[1].tolist()                            # radius2 = d - 1 ulp: d = next float above: out
        _assert_same(at, range_oracle(q[i:i + 1], r, radius2), "inclusive")
        _assert_same(short, range_oracle(q[i:i + 1], r, below), "next float")


def test_identical_runs_straddle_chunk_round_and_wave_boundaries(pkg):
    k, m, n = 16, 5, 70001
    p = pkg.plan_range(k, m, n)
    assert p["chunks"] > 2
    per = p["per"]
    r = _rand(41, n, k)
    q = _rand(42, m, k)
    marks = [per - 70, 2 * per - 1, per + 256 - 30, per + 64 - 10, n - 100]
    for s in marks:
        r[s:s + 140] = r[5]
    q[1] = r[5]
    q[3] = r[5]
    for radius2 in (0.0, 0.05):
        want = range_oracle(q, r, radius2)
        _assert_same(_whole(pkg, q, r, radius2), want, f"runs r2={radius2}")
        got = _index_range(pkg, torch.from_numpy(r).to(DEV), torch.from_numpy(q).to(DEV), radius2)
        _assert_same(got, want, f"runs split r2={radius2}")
    lims = range_oracle(q, r, 0.0)[0]
    assert lims[2] - lims[1] >= 4 * 140


def test_one_query_hits_everything_tile_mates_nothing(pkg):
    k, m, n = 8, 16, 9000
    q = _rand(51, m, k) + np.float32(100)
    r = _rand(52, n, k)
    q[6] = np.float32(0.5)
    radius2 = float(v0_all(q[6:7], r).max())
    want = range_oracle(q, r, radius2)
    assert want[0][7] - want[0][6] == n and want[0][-1] == n
    _assert_same(_whole(pkg, q, r, radius2), want, "flood")
    got = _index_range(pkg, torch.from_numpy(r).to(DEV), torch.from_numpy(q).to(DEV), radius2, path="exact")
    _assert_same(got, want, "flood split")


# ---- 4. non-finite data, overflow, radius2 = +INF and 0 -----------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_nonfinite_overflow_and_special_radii(pkg, bf16):
    k, m, n = 5, 30, 4000
    q = _rand(61, m, k)
    r = _rand(62, n, k)
    r[::7, 1] = np.nan
    r[1::7, 2] = np.inf
    r[2::7, 0] = -np.inf
    r[3::7, 4] = 3e19                  # squares overflow to +INF
    q[3, 2] = np.nan
    q[4, 0] = np.inf
    q[5, 1] = 1e30
    q[8] = r[20]
    r[3000] = r[20]
    q, r = _as_searched(pkg, q, bf16), _as_searched(pkg, r, bf16)
    for radius2 in (0.0, -0.0, 0.2, 3e38, INF):
        want = range_oracle(q, r, radius2)
        _assert_same(_whole(pkg, q, r, radius2, bf16), want, f"nonfinite r2={radius2} bf16={bf16}")
        got = _index_range(pkg, _to_dev(pkg, r, bf16), _to_dev(pkg, q, bf16), radius2)
        _assert_same(got, want, f"nonfinite split r2={radius2} bf16={bf16}")
    lims, idx, _ = range_oracle(q, r, 0.0)
    assert idx[lims[8]:lims[9]].tolist() == [20, 3000]             # radius2 = 0: exact duplicates only
    assert lims[4] - lims[3] == 0 and lims[5] - lims[4] == 0       # NaN / INF query: no hit


# ---- 5. cross-checks with the existing features ------------------------------------------------------------------
def test_contains_topk_at_the_kn_th_distance(pkg):
    k, m, n, kn = 16, 24, 20000, 10
    q = _rand(71, m, k)
    r = _rand(72, n, k)
    r[500:520] = r[9]
    q[2] = r[9]
    tidx, tdist = pkg.search_topk(q, r, kn, return_distances=True)
    for i in range(m):
        lims, idx, dist = pkg.search_range(q[i:i + 1], r, float(tdist[i, -1]), return_distances=True)
        assert set(tidx[i].tolist()) <= set(idx.tolist()), i
        assert np.array_equal(_bits(np.sort(dist)[:kn]), _bits(tdist[i])), i
    lims, idx = pkg.search_range(q[:1], r, INF)
    assert lims.tolist() == [0, n] and np.array_equal(idx, np.arange(n))


def test_infinite_radius_counts_finite_refs(pkg):
    k, n = 4, 6000
    q = _rand(81, 1, k)
    r = _rand(82, n, k)
    r[::5, 0] = np.nan
    r[1::9, 3] = 2e19                  # +INF distance
    finite = int(np.isfinite(v0_all(q, r)).sum())
    lims, idx = pkg.search_range(q, r, INF)
    assert lims.tolist() == [0, finite]


# ---- 6. index paths, SoA refs, index_base, streams, device ------------------------------------------------------
@pytest.mark.parametrize("path", ["auto", "exact", "mfma"])
def test_index_paths_soa_and_base(pkg, path):
    k, m, n = 32, 70, 5000
    q = _rand(91, m, k)
    r = _rand(92, n, k)
    radius2 = _radii(v0_all(q, r), n)[2]
    base = 2 ** 31 - 1 - n
    want = range_oracle(q, r, radius2, index_base=base)
    qd = torch.from_numpy(q).to(DEV)
    _assert_same(_index_range(pkg, torch.from_numpy(r).to(DEV), qd, radius2, path=path, index_base=base), want,
                 f"path={path}")
    soa = torch.from_numpy(np.ascontiguousarray(r.T)).to(DEV)
    _assert_same(_index_range(pkg, soa, qd, radius2, path=path, index_base=base, soa=True), want, f"soa path={path}")
    _assert_same(pkg.search_range(np.ascontiguousarray(q), np.ascontiguousarray(r.T), radius2, return_distances=True,
                                  refs_soa=True), range_oracle(q, r, radius2), "whole soa")
    qb, rb = _as_searched(pkg, q, True), _as_searched(pkg, r, True)
    _assert_same(_index_range(pkg, _to_dev(pkg, rb, True), _to_dev(pkg, qb, True), radius2, path=path,
                              index_base=base), range_oracle(qb, rb, radius2, index_base=base), f"bf16 path={path}")


def test_caller_stream_and_device_restored(pkg):
    k, m, n = 16, 40, 8000
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
    ix = pkg.Index(rd, stream=s)
    lims, idx, dist = ix.search_range(qd, radius2, return_distances=True, stream=s)
    s.synchronize()
    _assert_same((lims.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy()), want, "caller stream")
    ix.close()
    _whole(pkg, q, r, radius2)
    assert torch.cuda.current_device() == dev_before


# ---- 7. the count / fill contract ------------------------------------------------------------------------------
def test_searches_between_count_and_fill(pkg):
    k, m, n = 16, 50, 30000
    q = _rand(111, m, k)
    r = _rand(112, n, k)
    radius2 = _radii(v0_all(q, r), n)[2]
    want = range_oracle(q, r, radius2)
    qd, rd = torch.from_numpy(q).to(DEV), torch.from_numpy(r).to(DEV)
    q2 = torch.from_numpy(_rand(113, 300, k)).to(DEV)
    ix = pkg.Index(rd, path="exact")
    ref_keys = ix.search_keys(q2).clone()
    ref_topk = ix.search_topk_keys(q2, 7).clone()
    lims = ix.range_count(qd, radius2)
    keys = ix.search_keys(q2)                  # 1-NN and top-K of other queries in between
    tk = ix.search_topk_keys(q2, 7)
    total = int(lims[-1].item())
    idx = torch.full((total,), -7, dtype=torch.int32, device=DEV)
    dist = torch.full((total,), -1.0, dtype=torch.float32, device=DEV)
    ix.range_fill(qd, radius2, lims, idx=idx, dist=dist, return_distances=True)
    torch.cuda.synchronize()
    _assert_same((lims.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy()), want, "interleaved")
    assert torch.equal(keys, ref_keys) and torch.equal(tk, ref_topk)
    # a second fill of the same count gives identical buffers (positions come from counts)
    idx2 = ix.range_fill(qd, radius2, lims, total=total)
    torch.cuda.synchronize()
    assert torch.equal(idx2, idx)
    ix.close()


def test_fill_must_match_the_last_count(pkg):
    k, m, n = 3, 20, 5000
    qd = torch.from_numpy(_rand(121, m, k)).to(DEV)
    rd = torch.from_numpy(_rand(122, n, k)).to(DEV)
    ix = pkg.Index(rd)
    idx = torch.empty(m * n, dtype=torch.int32, device=DEV)
    lims = torch.zeros(m + 1, dtype=torch.int64, device=DEV)
    L = pkg.lib
    assert L.nns_index_range_fill(ix._h, m, qd.data_ptr(), 0.01, lims.data_ptr(), idx.data_ptr(), None, None) == 1
    ix.range_count(qd, 0.01, lims=lims)
    assert L.nns_index_range_fill(ix._h, m - 1, qd.data_ptr(), 0.01, lims.data_ptr(), idx.data_ptr(), None, None) == 1
    assert L.nns_index_range_fill(ix._h, m, qd.data_ptr(), 0.02, lims.data_ptr(), idx.data_ptr(), None, None) == 1
    other = qd.clone()
    assert L.nns_index_range_fill(ix._h, m, other.data_ptr(), 0.01, lims.data_ptr(), idx.data_ptr(), None, None) == 1
    assert b"last nns_index_range_count" in L.nns_last_error()
    assert L.nns_index_range_fill(ix._h, m, qd.data_ptr(), 0.01, lims.data_ptr(), idx.data_ptr(), None, None) == 0
    ix.range_count(other, 0.01, lims=lims)       # another count in between: the first one's fill is refused
    assert L.nns_index_range_fill(ix._h, m, qd.data_ptr(), 0.01, lims.data_ptr(), idx.data_ptr(), None, None) == 1
    assert L.nns_index_range_count(ix._h, m, qd.data_ptr(), float("nan"), lims.data_ptr(), None) == 1
    assert L.nns_index_range_count(ix._h, m, qd.data_ptr(), -0.5, lims.data_ptr(), None) == 1
    assert L.nns_index_range_fill(ix._h, m, other.data_ptr(), 0.01, lims.data_ptr(), idx.data_ptr(), None, None) == 1
    torch.cuda.synchronize()
    ix.close()


# ---- 8. whole call, split API and shards ------------------------------------------------------------------------
def test_whole_equals_split_and_shards_concatenate(pkg):
    k, m, n = 16, 45, 33333
    q = _rand(131, m, k)
    r = _rand(132, n, k)
    r[16600:16700] = r[3]
    q[0] = r[3]
    radius2 = _radii(v0_all(q, r), n)[2]
    want = range_oracle(q, r, radius2)
    whole = _whole(pkg, q, r, radius2)
    _assert_same(whole, want, "whole")
    qd = torch.from_numpy(q).to(DEV)
    _assert_same(_index_range(pkg, torch.from_numpy(r).to(DEV), qd, radius2), whole, "split")
    lims_w, idx_w = pkg.search_range(q, r, radius2)                # without distances
    assert np.array_equal(lims_w, whole[0]) and np.array_equal(idx_w, whole[1])
    h = pkg.shard_range(n, 2, 0)[1]
    parts = [_index_range(pkg, torch.from_numpy(r[beg:beg + cnt]).to(DEV), qd, radius2, index_base=beg)
             for beg, cnt in (pkg.shard_range(n, 2, s) for s in range(2))]
    assert h == pkg.shard_range(n, 2, 1)[0]
    idx = np.concatenate([np.concatenate([p[1][p[0][i]:p[0][i + 1]] for p in parts]) for i in range(m)])
    dist = np.concatenate([np.concatenate([p[2][p[0][i]:p[0][i + 1]] for p in parts]) for i in range(m)])
    lims = parts[0][0] + parts[1][0]
    _assert_same((lims, idx, dist), want, "shards")


def test_deterministic_buffers(pkg):
    k, m, n = 3, 1024, 200000
    qd = torch.empty((m, k), dtype=torch.float32, device=DEV)
    rd = torch.empty((n, k), dtype=torch.float32, device=DEV)
    pkg.fill_uniform(qd, 5, 0)
    pkg.fill_uniform(rd, 6, 0)
    ix = pkg.Index(rd)
    a = ix.search_range(qd, 0.003, return_distances=True)
    b = ix.search_range(qd, 0.003, return_distances=True)
    torch.cuda.synchronize()
    assert int(a[0][-1]) > 50 * m
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    qh, rh = qd.cpu().numpy(), rd.cpu().numpy()
    sel = [0, 1, 511, 1023]
    want = range_oracle(qh[sel], rh, 0.003)
    lims = a[0].cpu().numpy()
    idx, dist = a[1].cpu().numpy(), a[2].cpu().numpy()
    got_i = np.concatenate([idx[lims[i]:lims[i + 1]] for i in sel])
    got_d = np.concatenate([dist[lims[i]:lims[i + 1]] for i in sel])
    got_l = np.concatenate([[0], np.cumsum([lims[i + 1] - lims[i] for i in sel])])
    _assert_same((got_l, got_i, got_d), want, "large")
    ix.close()


# ---- 9. a total above 2^31 -------------------------------------------------------------------------------------
def test_total_above_2_31(pkg):
    m, n = 2100, 1 << 20
    qd = torch.empty((m, 1), dtype=torch.float32, device=DEV)
    rd = torch.empty((n, 1), dtype=torch.float32, device=DEV)
    pkg.fill_uniform(qd, 7, 0)
    pkg.fill_uniform(rd, 8, 0)
    ix = pkg.Index(rd)
    lims = ix.range_count(qd, INF)
    total = int(lims[-1].item())
    assert total == m * n > 2 ** 31
    assert torch.equal(lims, torch.arange(m + 1, dtype=torch.int64, device=DEV) * n)
    idx = torch.empty(total, dtype=torch.int32, device=DEV)
    ix.range_fill(qd, INF, lims, idx=idx)
    torch.cuda.synchronize()
    ar = torch.arange(n, dtype=torch.int32, device=DEV)
    for i in (0, 1, 1023, 2047, 2048, 2099):             # rows that start below and above 2^31
        assert torch.equal(idx[i * n:(i + 1) * n], ar), i
    ix.close()
    del idx


# ---- 10. statistics -------------------------------------------------------------------------------------------
def test_stats_report_the_exact_path(pkg):
    k, m, n = 64, 100, 20000
    qd = torch.from_numpy(_rand(141, m, k)).to(DEV)
    rd = torch.from_numpy(_rand(142, n, k)).to(DEV)
    ix = pkg.Index(rd, path="mfma", profile=True)
    ix.search_keys(qd)
    assert ix.stats()["path"] == 2
    ix.search_range(qd, 5.0)
    st = ix.stats()
    assert st["path"] == 1
    assert st["exact_ms"] > 0 and st["total_ms"] > 0
    ix.close()
    lims, idx = pkg.search_range(qd.cpu().numpy(), rd.cpu().numpy(), 5.0, path="exact")
    assert lims[-1] == len(idx)


# ---- 11. no hits through the split API ----------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_zero_hits_split_api(pkg, bf16):
    k, m, n = 16, 40, 3000
    q = _as_searched(pkg, _rand(151, m, k) + np.float32(10), bf16)    # far from every ref
    r = _as_searched(pkg, _rand(152, n, k), bf16)
    qd, rd = _to_dev(pkg, q, bf16), _to_dev(pkg, r, bf16)
    for radius2 in (0.0, 1.0):
        want = range_oracle(q, r, radius2)
        assert want[0][-1] == 0
        got = _index_range(pkg, rd, qd, radius2)
        _assert_same(got, want, f"no hits r2={radius2}")
        assert got[1].shape == (0,) and got[2].shape == (0,)
        _assert_same(_whole(pkg, q, r, radius2, bf16), want, f"no hits whole r2={radius2}")
    ix = pkg.Index(rd)
    lims = ix.range_count(qd, 0.0)
    idx, dist = ix.range_fill(qd, 0.0, lims, return_distances=True)      # zero-size tensors: null pointers
    torch.cuda.synchronize()
    assert idx.numel() == 0 and dist.numel() == 0 and not torch.any(lims)
    assert pkg.lib.nns_index_range_fill(ix._h, m, qd.data_ptr(), 0.0, lims.data_ptr(), None, None, None) == 0
    ix.close()


# ---- 12. the lims scan over several tiles, and query groups beyond one grid row --------------------------------
def test_multi_tile_lims_scan(pkg):
    k, m, n = 1, 10000, 5000                     # 3 scan tiles of 4096 counts, several ref chunks
    p = pkg.plan_range(k, m, n)
    assert p["chunks"] > 1
    q = _rand(161, m, k)
    r = _rand(162, n, k)
    q[5000:5100] = r[17]
    for radius2 in (0.0, 1e-4, 0.01):
        want = range_oracle(q, r, radius2)
        _assert_same(_whole(pkg, q, r, radius2), want, f"tiles whole r2={radius2}")
        got = _index_range(pkg, torch.from_numpy(r).to(DEV), torch.from_numpy(q).to(DEV), radius2)
        _assert_same(got, want, f"tiles split r2={radius2}")


def _device_lims_1d(qd, rd, radius2):
    """lims of a 1-D search from torch on the device (one subtraction and one square per pair: V0's arithmetic)."""
    cnt = torch.zeros(qd.shape[0], dtype=torch.int64, device=DEV)
    for j in range(rd.shape[0]):
        diff = qd[:, 0] - rd[j, 0]
        cnt += (diff * diff <= radius2).to(torch.int64)
    return torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), torch.cumsum(cnt, 0)])


@pytest.mark.parametrize("m", [(1 << 24) + 3 * 4096 + 5, (1 << 28) + 3])
def test_many_queries(pkg, m):
    # m = 2^24 + ...: more than 4096 scan tiles (the tile-sum scan takes several steps);
    # m = 2^28 + 3: 2^24 + 1 query groups of 16, more than one grid row of workgroups holds
    qd = torch.empty((m, 1), dtype=torch.float32, device=DEV)
    pkg.fill_uniform(qd, 171, 0)
    rd = torch.tensor([[0.25], [0.5], [0.7]], dtype=torch.float32, device=DEV)
    radius2 = 0.01
    ix = pkg.Index(rd)
    lims = ix.range_count(qd, radius2)
    want = _device_lims_1d(qd, rd, radius2)
    assert torch.equal(lims, want)
    total = int(lims[-1].item())
    idx = torch.empty(total, dtype=torch.int32, device=DEV)
    ix.range_fill(qd, radius2, lims, idx=idx)
    torch.cuda.synchronize()
    lh = lims.cpu().numpy()
    qh = qd[:, 0].cpu().numpy()
    rng = np.random.default_rng(172)
    rows = np.concatenate([[0, 1, m - 2, m - 1], rng.integers(0, m, 2000)])
    for i in rows:
        d = (qh[i] - np.array([0.25, 0.5, 0.7], np.float32)) ** 2
        want_i = np.nonzero(d <= np.float32(radius2))[0]
        assert idx[lh[i]:lh[i + 1]].cpu().numpy().tolist() == want_i.tolist(), i
    ix.close()
    del idx, lims, want, qd
