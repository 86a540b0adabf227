"""GPU tests of the MFMA-filtered top-K search (NNS_TOPK_MFMA, K6m): indices exact and distance bits equal to the numpy
top-K oracle of test_topk_cpu.py on every shape, through the split API of a flagged index and the whole call — a grid
over k, both ref image layouts, several ring slots / splits / chunks and block edges, kn = 256, ties, queue flushes on
every round, samples that say nothing about the rest of the refs, bounds on the number of flagged blocks, re-scaled
data, non-finite queries and refs, the fall-backs, index options, determinism, the caller's stream and query batches."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_range_cpu import v0_all  # noqa: E402
from test_topk_cpu import topk_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
EXACT, MFMA = 1, 2


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_same(got, want, what):
    idx, dist = got
    want_idx, want_dist = want
    bad = np.argwhere(idx != want_idx)
    assert bad.size == 0, f"{what}: {len(bad)} index mismatches, first at {bad[:3].tolist()}"
    assert np.array_equal(_bits(dist), _bits(want_dist)), f"{what}: distance bits differ"


def _rand(seed, *shape):
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _search(pkg, ix, qd, kn, stream=None):
    """((idx, dist) on the host, topk_info) of one split-API top-K search."""
    keys = ix.search_topk_keys(qd, kn, stream=stream)
    idx, dist = pkg.keys_topk_unpack(keys, return_distances=True, stream=stream)
    torch.cuda.synchronize()
    return (idx.cpu().numpy(), dist.cpu().numpy()), ix.topk_info()


def _cut(want, kn):
    """the first kn columns of an oracle answer: rows are in (distance, index) order, so a prefix is the smaller top-K"""
    return want[0][:, :kn], want[1][:, :kn]


def _nblk(n):
    return -(-n // 32)


# ---- 1. a grid over k -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 16, 24, 64, 100, 128, 200, 256])
def test_grid(pkg, k):
    m, n = 130, 6000
    q = _rand(10 + k, m, k)
    r = _rand(20 + k, n, k)
    r[100:140] = r[7]                                    # a run of equal distances for every query
    want10 = topk_oracle(q, r, 10)
    ix = pkg.Index(_dev(r), topk_mfma=True)
    qd = _dev(q)
    for kn in (1, 10):
        assert pkg.plan_topk_mfma(k, m, n, kn)["filtered"] == 1
        want = _cut(want10, kn)
        got, info = _search(pkg, ix, qd, kn)
        _assert_same(got, want, f"split k={k} kn={kn}")
        assert info["path"] == MFMA and info["examined"] == m * pkg.plan_range_mfma(k, m, n)["blocks_per_query"], info
        assert 0 < info["flagged"] <= m * _nblk(n) and info["filled"] == 0, info
        assert ix.stats()["path"] == MFMA
        _assert_same(pkg.search_topk(q, r, kn, return_distances=True, topk_mfma=True), want, f"whole k={k} kn={kn}")
    keys1 = ix.search_topk_keys(qd, 1)
    assert torch.equal(keys1[:, 0], ix.search_keys(qd))  # kn = 1: the 1-NN search's keys
    ix.close()


# ---- 2. both image layouts ------------------------------------------------------------------------------------
@pytest.mark.parametrize("eager", [False, True], ids=["default", "eager"])
@pytest.mark.parametrize("k", [64, 128])
def test_both_image_layouts(pkg, k, eager):
    m, n, kn = 70, 5000, 5
    lazy_depth = pkg.plan_filter(k, 65536, 1 << 20, schedule=True)["lazy"] == 1
    p = pkg.plan_topk_mfma(k, m, n, kn, pkg.NNS_FILTER_SPLIT_EAGER if eager else 0)
    assert p["filtered"] == 1 and p["layout"] == int(lazy_depth and not eager)
    if k == 128:
        assert p["layout"] == int(not eager)             # the lazy depth: both layouts are reached
    q = _rand(31 + k, m, k)
    r = _rand(32 + k, n, k)
    ix = pkg.Index(_dev(r), topk_mfma=True, filter_split_eager=eager)
    got, info = _search(pkg, ix, _dev(q), kn)
    _assert_same(got, topk_oracle(q, r, kn), f"k={k} eager={eager}")
    assert info["path"] == MFMA
    ix.close()


# ---- 3. several ring slots, splits and chunks; block, flag-word and chunk edges --------------------------------
@pytest.fixture(scope="module")
def edges():
    k, m, n = 16, 600, 70001
    q = _rand(41, m, k)
    r = _rand(42, n, k)
    return k, m, n, q, r, topk_oracle(q, r, 100)


@pytest.mark.parametrize("kn", [16, 100])
def test_slots_splits_chunks_and_block_edges(pkg, edges, kn):
    k, m, n, q, r0, want100 = edges
    p = pkg.plan_topk_mfma(k, m, n, kn)
    assert p["filtered"] == 1 and p["grid_x"] == 2 and p["grid_y"] > 1 and p["chunks"] == 2 and p["chunk_words"] == 64
    s = p["stride"]
    assert s >= 3
    # near-duplicates of queries at block edges, the last block, a flag-word edge (blocks 31 | 32), the chunk edge
    # (blocks 2047 | 2048), and in a sampled block (s) and the unsampled ones around it
    spots = (0, 31, 32, n - 1, n - 9, 32 * 32 - 1, 32 * 32, 2047 * 32 + 5, 2048 * 32, s * 32 + 3, (s - 1) * 32 + 31,
             (s + 1) * 32)
    assert {j // 32 % s == 0 for j in spots} == {True, False}
    r = r0.copy()
    for i, j in enumerate(spots):
        r[j] = q[7 * i]
        r[j][0] += np.float32(1e-3)
    # the oracle's rows change only where a planted ref enters or the ref it replaced leaves: recompute those queries
    want = [w[:, :kn].copy() for w in want100]
    d = v0_all(q, r[list(spots)])                        # distances to the planted refs
    enters = (d <= want100[1][:, kn - 1:kn]).any(axis=1)
    leaves = np.isin(want[0], spots).any(axis=1)
    touched = np.flatnonzero(enters | leaves)
    assert set(range(0, 7 * len(spots), 7)) <= set(touched.tolist()) and len(touched) < 100
    redo = topk_oracle(q[touched], r, kn)
    want[0][touched], want[1][touched] = redo
    ix = pkg.Index(_dev(r), topk_mfma=True)
    got, info = _search(pkg, ix, _dev(q), kn)
    _assert_same(got, want, f"edges kn={kn}")
    for i, j in enumerate(spots):
        assert j in got[0][7 * i].tolist(), (i, j)
    print(f"kn={kn}: flagged {info['flagged']} of {info['examined']}")
    assert info["path"] == MFMA and info["filled"] == 0
    if kn == 16:
        assert 0 < info["flagged"] < info["examined"] // 4
    _assert_same(pkg.search_topk(q, r, kn, return_distances=True, topk_mfma=True), want, f"whole edges kn={kn}")
    ix.close()


# ---- 4. the longest lists -------------------------------------------------------------------------------------
def test_kn_256(pkg):
    k, m, n, kn = 16, 64, 140000, 256
    assert pkg.plan_topk_mfma(k, m, n, kn)["stride"] == 4
    q = _rand(51, m, k)
    r = _rand(52, n, k)
    ix = pkg.Index(_dev(r), topk_mfma=True)
    got, info = _search(pkg, ix, _dev(q), kn)
    _assert_same(got, topk_oracle(q, r, kn), "kn=256")
    assert info["path"] == MFMA
    ix.close()


# ---- 5. ties --------------------------------------------------------------------------------------------------
def test_ties_at_the_kth_distance(pkg):
    k, m, n, kn = 16, 64, 70001, 100
    q = _rand(61, m, k)
    r = _rand(62, n, k)
    r[1000:1300] = q[0]                                  # 300 copies of query 0: the lowest 100 indices win
    ix = pkg.Index(_dev(r), topk_mfma=True)
    got, info = _search(pkg, ix, _dev(q), kn)
    assert info["path"] == MFMA
    assert got[0][0].tolist() == list(range(1000, 1100)) and not got[1][0].any()
    _assert_same(got, topk_oracle(q, r, kn), "copies")
    ix.close()
    n = 60000
    r = np.tile(_rand(63, 1, k), (n, 1))                 # all refs equal: every distance of a query ties
    ix = pkg.Index(_dev(r), topk_mfma=True)
    got, info = _search(pkg, ix, _dev(q), kn)
    assert info["path"] == MFMA
    assert np.array_equal(got[0], np.tile(np.arange(kn, dtype=np.int32), (m, 1)))
    want_d = v0_all(q, r[:1])                            # one distance per query
    assert np.array_equal(_bits(got[1]), _bits(np.tile(want_d, (1, kn))))
    ix.close()


# ---- 6. a flush on every round --------------------------------------------------------------------------------
@pytest.mark.parametrize("far_sample", [False, True], ids=["cluster", "cluster_far_sample"])
@pytest.mark.parametrize("kn", [7, 256])
def test_flush_stress(pkg, kn, far_sample):
    """A tight cluster ordered farthest-first for query 0: every ref it meets beats the threshold of the moment.  The
    refs are centred before the filter sees them, so the flag pass still tells the cluster's blocks apart and query 0
    meets only some of them; with the sampled blocks moved away (far_sample) the bound is loose, every block of every
    query is flagged, and the queue of query 0 fills and flushes round after round over all the other refs."""
    k, m, n = 16, 64, 40000
    p = pkg.plan_topk_mfma(k, m, n, kn)
    assert p["filtered"] == 1
    c = np.float32(0.5)
    r = (c + np.float32(1e-6) * _rand(71, n, k)).astype(np.float32)
    q = (c + np.float32(1e-6) * _rand(72, m, k)).astype(np.float32)
    q[0] = c
    order = np.argsort(-v0_all(q[:1], r)[0], kind="stable")
    r = np.ascontiguousarray(r[order])
    if far_sample:
        r[(np.arange(n) // 32) % p["stride"] == 0] += np.float32(1)
    ix = pkg.Index(_dev(r), topk_mfma=True)
    got, info = _search(pkg, ix, _dev(q), kn)
    _assert_same(got, topk_oracle(q, r, kn), f"flush stress kn={kn} far_sample={far_sample}")
    print(f"kn={kn} far_sample={far_sample}: flagged {info['flagged']} of {info['examined']}")
    assert info["path"] == MFMA and info["flagged"] > 0
    if far_sample:
        assert info["flagged"] == m * _nblk(n)           # every block holds a ref within the bound
    ix.close()


# ---- 7. a sample that says nothing about the other refs -------------------------------------------------------
@pytest.mark.parametrize("sample_far", [True, False], ids=["sample_far", "sample_near"])
def test_unrepresentative_sample(pkg, sample_far):
    k, m, n, kn = 16, 64, 20000, 10
    p = pkg.plan_topk_mfma(k, m, n, kn)
    assert p["filtered"] == 1 and p["stride"] >= 2
    q = _rand(81, m, k)
    r = _rand(82, n, k)
    sampled = (np.arange(n) // 32) % p["stride"] == 0
    r[sampled if sample_far else ~sampled] += np.float32(10)
    ix = pkg.Index(_dev(r), topk_mfma=True)
    got, info = _search(pkg, ix, _dev(q), kn)
    _assert_same(got, topk_oracle(q, r, kn), f"sample_far={sample_far}")
    assert info["path"] == MFMA
    if not sample_far:
        assert np.all(sampled[got[0]])                   # the answers are the sample's own
    ix.close()


# ---- 8. the number of flagged blocks lies between the model's bounds ------------------------------------------
def test_flag_bounds(pkg):
    """With U_i the kn-th smallest V0 distance over the plan's sample: every block holding a ref with d <= U_i is
    flagged, and a flagged block holds a ref with d <= U_i + 2 tau(U_i - |x'|^2) (K7m's threshold is a + 1.002 tau(a)
    and a score lies within tau / 2 of d - |x'|^2; test_range_mfma_gpu.py's test_flag_bounds).  Norms of the centred
    points are recomputed in fp64 around the fp32-rounded column mean; 1e-5 relative on the upper radius covers the
    mean's rounding."""
    k, m, n, kn = 64, 128, 20000, 10
    p = pkg.plan_topk_mfma(k, m, n, kn)
    assert p["filtered"] == 1
    q = _rand(91, m, k)
    r = _rand(92, n, k)
    d = v0_all(q, r)
    sampled = (np.arange(n) // 32) % p["stride"] == 0
    assert sampled.sum() == p["sample_refs"]
    U = np.sort(d[:, sampled], axis=1)[:, kn - 1]
    c = r.astype(np.float64).mean(axis=0).astype(np.float32)
    qn = ((q - c).astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
    ymax2 = float(((r - c).astype(np.float64) ** 2).sum(axis=1).max().astype(np.float32))
    nblk = _nblk(n)
    dpad = np.full((m, nblk * 32), np.inf, np.float32)
    dpad[:, :n] = d
    bmin = dpad.reshape(m, nblk, 32).min(axis=2)         # the nearest ref of every (query, block)
    lo = int((bmin <= U[:, None]).sum())
    hi = 0
    for i in range(m):
        c0, c1, x2 = pkg.tau_consts(p["kt"], float(qn[i]), ymax2, 3)
        tau = c0 + c1 * max(float(U[i]) - float(qn[i]) + x2, 0.0)
        hi += int((bmin[i].astype(np.float64) <= (float(U[i]) + 2.0 * tau) * (1.0 + 1e-5)).sum())
    ix = pkg.Index(_dev(r), topk_mfma=True)
    got, info = _search(pkg, ix, _dev(q), kn)
    _assert_same(got, topk_oracle(q, r, kn), "flag bounds")
    print(f"flagged {info['flagged']} of {info['examined']} (lo {lo}, hi {hi})")
    assert info["path"] == MFMA and info["examined"] == m * p["blocks_per_query"]
    assert lo <= info["flagged"] <= hi, (lo, info, hi)
    ix.close()


# ---- 9. underflow and large scale -----------------------------------------------------------------------------
@pytest.mark.parametrize("exp", [-60, 40])
def test_scaled_data(pkg, exp):
    k, m, n, kn = 16, 130, 6000, 10
    s = np.float32(2.0 ** exp)
    q = _rand(10 + k, m, k) * s                          # test 1's data, re-scaled exactly
    r = _rand(20 + k, n, k) * s
    r[100:140] = r[7]
    ix = pkg.Index(_dev(r), topk_mfma=True)
    got, info = _search(pkg, ix, _dev(q), kn)
    _assert_same(got, topk_oracle(q, r, kn), f"scale 2^{exp}")
    assert info["path"] == MFMA
    ix.close()


# ---- 10. non-finite values and the fall-backs -----------------------------------------------------------------
def test_nonfinite_queries_refs_and_fallbacks(pkg):
    k, m, n, kn = 16, 72, 6000, 10
    q = _rand(101, m, k)
    r = _rand(102, n, k)
    q[5, 3] = np.nan
    q[17, 0] = np.inf
    q[40, 0] = 1e17
    want = topk_oracle(q, r, kn)
    assert np.all(want[0][[5, 17]] == -1) and np.all(np.isinf(want[1][[5, 17]])) and np.all(want[0][40] >= 0)
    ix = pkg.Index(_dev(r), topk_mfma=True)
    got, info = _search(pkg, ix, _dev(q), kn)
    _assert_same(got, want, "void queries")
    assert info["path"] == MFMA and info["filled"] == 3, info
    assert 3 * _nblk(n) <= info["flagged"] < m * _nblk(n), info     # three filled rows; the rest filtered
    got, info = _search(pkg, ix, _dev(q[:63]), kn)       # below the filter's query floor
    _assert_same(got, _cut((want[0][:63], want[1][:63]), kn), "63 queries")
    assert info == {"path": EXACT, "flagged": 0, "examined": 0, "filled": 0} and ix.stats()["path"] == EXACT
    ix.close()
    ix = pkg.Index(_dev(r[:3000]), topk_mfma=True)       # too few refs for a sample with stride 2
    assert pkg.plan_topk_mfma(k, m, 3000, kn)["filtered"] == 0
    got, info = _search(pkg, ix, _dev(q), kn)
    _assert_same(got, topk_oracle(q, r[:3000], kn), "small n")
    assert info["path"] == EXACT
    ix.close()
    r[77, 2] = np.nan                                    # refs_bad
    ix = pkg.Index(_dev(r), topk_mfma=True)
    got, info = _search(pkg, ix, _dev(q), kn)
    _assert_same(got, topk_oracle(q, r, kn), "nan ref")
    assert info["path"] == EXACT and ix.stats()["path"] == EXACT
    ix.close()


# ---- 11. index behaviour --------------------------------------------------------------------------------------
def test_index_base_and_refresh(pkg):
    k, m, n, kn, base = 32, 70, 6000, 8, 10 ** 6
    q = _rand(111, m, k)
    r = _rand(112, n, k)
    want = topk_oracle(q, r, kn)
    rd, qd = _dev(r), _dev(q)
    for path in ("auto", "exact"):
        ix = pkg.Index(rd, path=path, index_base=base, topk_mfma=True)
        got, info = _search(pkg, ix, qd, kn)
        _assert_same(got, (want[0] + base, want[1]), f"index_base path={path}")
        assert info["path"] == MFMA
        ix.close()
    ix = pkg.Index(rd, topk_mfma=True)
    r2 = _rand(113, n, k)
    rd.copy_(_dev(r2))                                   # rewritten in place
    ix.refresh()
    got, info = _search(pkg, ix, qd, kn)
    _assert_same(got, topk_oracle(q, r2, kn), "refreshed")
    assert info["path"] == MFMA
    r2[5, 5] = np.inf
    rd.copy_(_dev(r2))
    ix.refresh()
    got, info = _search(pkg, ix, qd, kn)                 # the refresh is looked at before the filtered path is taken
    _assert_same(got, topk_oracle(q, r2, kn), "refreshed, inf ref")
    assert info["path"] == EXACT
    ix.close()


def test_interleaved_with_nearest_and_range_passes(pkg):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_range_cpu import range_oracle
    k, m, n, kn = 16, 80, 30000, 12
    q = _rand(121, m, k)
    r = _rand(122, n, k)
    d = v0_all(q, r)
    radius2 = float(np.sort(d.ravel())[3 * m])
    want_range = range_oracle(q, r, radius2)
    want = topk_oracle(q, r, kn)
    qd = _dev(q)
    ix = pkg.Index(_dev(r), path="mfma", range_mfma=True, topk_mfma=True)
    ref_keys = ix.search_keys(qd).clone()
    lims = ix.range_count(qd, radius2)
    assert ix.range_info()["path"] == MFMA
    got, info = _search(pkg, ix, qd, kn)                 # a filtered top-K between count and fill: it takes the bitmap
    _assert_same(got, want, "between count and fill")
    assert info["path"] == MFMA
    assert torch.equal(ix.search_keys(qd), ref_keys)
    idx, dist = ix.range_fill(qd, radius2, lims, return_distances=True)
    torch.cuda.synchronize()
    assert np.array_equal(lims.cpu().numpy(), want_range[0]) and np.array_equal(idx.cpu().numpy(), want_range[1])
    assert np.array_equal(_bits(dist.cpu().numpy()), _bits(want_range[2]))
    assert ix.range_info()["hits"] == want_range[0][-1] and ix.topk_info() == info
    got, info = _search(pkg, ix, qd, kn)
    _assert_same(got, want, "after the fill")
    assert torch.equal(ix.search_keys(qd), ref_keys)
    ix.close()


def test_deterministic_buffers(pkg):
    k, m, n, kn = 16, 256, 50000, 20
    qd = torch.empty((m, k), dtype=torch.float32, device=DEV)
    rd = torch.empty((n, k), dtype=torch.float32, device=DEV)
    pkg.fill_uniform(qd, 5, 0)
    pkg.fill_uniform(rd, 6, 0)
    ix = pkg.Index(rd, topk_mfma=True)
    runs = []
    for garbage in (-7, 0x5A5A5A5A):
        keys = torch.full((m, kn), garbage, dtype=torch.int64, device=DEV)
        ix.search_topk_keys(qd, kn, keys=keys)
        runs.append((keys.cpu().numpy().tobytes(), ix.topk_info()))
    assert runs[0] == runs[1] and runs[0][1]["path"] == MFMA
    ref = pkg.Index(rd, path="exact")
    assert torch.equal(ref.search_topk_keys(qd, kn), keys)           # K6's keys
    ref.close()
    ix.close()


def test_caller_stream_and_device_restored(pkg):
    k, m, n, kn = 16, 70, 12000, 6
    q = _rand(131, m, k)
    r = _rand(132, n, k)
    want = topk_oracle(q, r, kn)
    dev_before = torch.cuda.current_device()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        qd = torch.from_numpy(q).to(DEV)
        rd = torch.from_numpy(r).to(DEV)
    s.synchronize()
    ix = pkg.Index(rd, stream=s, topk_mfma=True)
    got, info = _search(pkg, ix, qd, kn, stream=s)
    _assert_same(got, want, "caller stream")
    assert info["path"] == MFMA
    ix.close()
    _assert_same(pkg.search_topk(q, r, kn, return_distances=True, topk_mfma=True, shards=2), want, "whole, two shards")
    assert torch.cuda.current_device() == dev_before


def test_profiled_index(pkg):
    """The stages of a filtered top-K pass are consecutive intervals between the events that bound total_ms — rerank_ms
    the bound scan, prep_queries_ms K2 on the queries, filter_ms the flag pass, finalize_ms the selection up to the
    pass's end event — so they add up to it but for the roundings of five elapsed times: 1e-5 relative, plus 1 us for
    each of the five read-outs (the resolution HIP documents for hipEventElapsedTime is around 0.5 us)."""
    k, m, n, kn = 16, 128, 40000, 8
    q = _rand(141, m, k)
    r = _rand(142, n, k)
    ix = pkg.Index(_dev(r), profile=True, topk_mfma=True)
    ix.stats()
    got, info = _search(pkg, ix, _dev(q), kn)
    _assert_same(got, topk_oracle(q, r, kn), "profiled")
    st = ix.stats()
    assert st["path"] == MFMA and info["path"] == MFMA, st
    stages = ("prep_queries_ms", "filter_ms", "finalize_ms", "rerank_ms")
    assert all(st[s] > 0.0 for s in stages) and st["exact_ms"] == 0.0, st
    assert abs(sum(st[s] for s in stages) - st["total_ms"]) <= 1e-5 * st["total_ms"] + 5e-3, st
    got, info = _search(pkg, ix, _dev(q[:32]), kn)       # the exact pass of the same index
    st = ix.stats()
    assert st["path"] == EXACT and info["path"] == EXACT and st["exact_ms"] > 0.0 and st["rerank_ms"] == 0.0, st
    ix.close()


# ---- 12. query batches ----------------------------------------------------------------------------------------
def test_two_query_batches(pkg):
    """2^20 queries x 70000 refs at k = 8 need 69 flag words per query: two batches under the 256 MiB cap.  Queries
    around the batch boundary and at both ends are held against the oracle."""
    k, m, n, kn = 8, 1 << 20, 70000, 2
    p = pkg.plan_topk_mfma(k, m, n, kn)
    assert p["filtered"] == 1 and p["batches"] == 2 and p["chunks"] == 1
    qd = torch.empty((m, k), dtype=torch.float32, device=DEV)
    rd = torch.empty((n, k), dtype=torch.float32, device=DEV)
    pkg.fill_uniform(qd, 15, 0)
    pkg.fill_uniform(rd, 16, 0)
    ix = pkg.Index(rd, topk_mfma=True)
    keys = ix.search_topk_keys(qd, kn)
    info = ix.topk_info()
    assert info["path"] == MFMA and info["examined"] == m * p["blocks_per_query"] and info["filled"] == 0
    assert 0 < info["flagged"] < info["examined"] // 4
    b = p["batch"]
    sel = [0, 1, b - 2, b - 1, b, b + 1, m - 2, m - 1]
    idx, dist = pkg.keys_topk_unpack(keys[sel].contiguous(), return_distances=True)
    torch.cuda.synchronize()
    _assert_same((idx.cpu().numpy(), dist.cpu().numpy()), topk_oracle(qd[sel].cpu().numpy(), rd.cpu().numpy(), kn),
                 "batch boundary")
    ix.close()
