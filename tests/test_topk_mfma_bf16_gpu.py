"""GPU tests of the MFMA-filtered top-K search for bf16 points (NNS_TOPK_MFMA on a bf16 index: K6's bound scan, the
16x16x32 flag kernel at the bounds, the selection on widened bf16 rows; 32 <= k <= 256).  Indices exact and distance
bits equal to the numpy top-K oracle of test_topk_cpu.py on the bf16 values widened to fp32, through the split API of a
flagged index and the whole call — a grid over k, several ring slots / splits / chunks and block edges, kn = 256, ties at
the kn-th distance, a sample that says nothing about the other refs, the fall-backs and the search's own report."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_range_gpu import _as_searched, _to_dev  # noqa: E402
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


def _pts(pkg, seed, *shape):
    """uniform [0, 1) values rounded to bf16, as fp32"""
    return _as_searched(pkg, np.random.default_rng(seed).random(shape, dtype=np.float32), True)


def _dev(pkg, a):
    return _to_dev(pkg, a, True)


def _search(pkg, ix, qd, kn):
    """((idx, dist) on the host, topk_info) of one split-API top-K search."""
    keys = ix.search_topk_keys(qd, kn)
    idx, dist = pkg.keys_topk_unpack(keys, return_distances=True)
    torch.cuda.synchronize()
    return (idx.cpu().numpy(), dist.cpu().numpy()), ix.topk_info()


def _whole(pkg, q, r, kn, **kw):
    return pkg.search_topk_bf16(pkg.to_bf16_bits(q), pkg.to_bf16_bits(r), kn, return_distances=True, topk_mfma=True, **kw)


def _cut(want, kn):
    """the first kn columns of an oracle answer: rows are in (distance, index) order, so a prefix is the smaller top-K"""
    return want[0][:, :kn], want[1][:, :kn]


def _nblk(n):
    return -(-n // 32)


# ---- (a) a grid over k; (g) the search's own report at k = 64 -----------------------------------------------------
@pytest.mark.parametrize("k", [32, 40, 64, 100, 128, 129, 200, 256])
def test_grid(pkg, k):
    # (kn = 100 leaves a stride of 2 from 12800 refs on.  The k = 64 case, whose report is held to "under a quarter of
    #  the blocks flagged" at every kn, has 100001 refs: with 13001 the stride-2 sample's 100th distance is the 200th of
    #  all refs, which over 407 blocks flags about a third of them whatever the filter does)
    m, n = 130, (100001 if k == 64 else 13001)
    q = _pts(pkg, 10 + k, m, k)
    r = _pts(pkg, 20 + k, n, k)
    r[100:140] = r[7]                                    # a run of equal distances for every query
    want100 = topk_oracle(q, r, 100)
    ix = pkg.Index(_dev(pkg, r), topk_mfma=True)
    qd = _dev(pkg, q)
    blocks = pkg.plan_range_mfma(k, m, n, bf16=True)["blocks_per_query"]
    for kn in (1, 10, 100):
        assert pkg.plan_topk_mfma(k, m, n, kn, bf16=True)["filtered"] == 1
        want = _cut(want100, kn)
        got, info = _search(pkg, ix, qd, kn)
        _assert_same(got, want, f"split k={k} kn={kn}")
        assert info["path"] == MFMA and info["examined"] == m * blocks, info
        assert 0 < info["flagged"] <= m * _nblk(n) and info["filled"] == 0, info
        assert ix.stats()["path"] == MFMA
        if k == 64:
            print(f"k=64 kn={kn}: flagged {info['flagged']} of {info['examined']}")
            assert 0 < info["flagged"] < info["examined"] // 4, info
        _assert_same(_whole(pkg, q, r, kn), want, f"whole k={k} kn={kn}")
    keys1 = ix.search_topk_keys(qd, 1)
    assert torch.equal(keys1[:, 0], ix.search_keys(qd))  # kn = 1: the 1-NN search's keys
    ix.close()


# ---- (b) several ring slots, splits and chunks; block, flag-word and chunk edges ----------------------------------
@pytest.fixture(scope="module")
def edges(pkg):
    k, m, n = 32, 600, 70001
    q = _pts(pkg, 41, m, k)
    r = _pts(pkg, 42, n, k)
    spots = (0, 31, 32, n - 1, n - 9, 2047 * 32 + 5, 2048 * 32)
    for i, j in enumerate(spots):
        r[j] = q[7 * i]                                  # exact duplicates of queries
    return k, m, n, q, r, spots, topk_oracle(q, r, 16)


@pytest.mark.parametrize("kn", [1, 16])
def test_slots_splits_chunks_and_block_edges(pkg, edges, kn):
    k, m, n, q, r, spots, want16 = edges
    p = pkg.plan_topk_mfma(k, m, n, kn, bf16=True)
    assert p["filtered"] == 1 and p["grid_x"] == 2 and p["grid_y"] > 1 and p["chunks"] == 2 and p["chunk_words"] == 64
    want = _cut(want16, kn)
    ix = pkg.Index(_dev(pkg, r), topk_mfma=True)
    got, info = _search(pkg, ix, _dev(pkg, q), kn)
    _assert_same(got, want, f"edges kn={kn}")
    for i, j in enumerate(spots):
        assert got[0][7 * i][0] == j and got[1][7 * i][0] == 0.0, (i, j)
    print(f"kn={kn}: flagged {info['flagged']} of {info['examined']}")
    assert info["path"] == MFMA and info["filled"] == 0 and 0 < info["flagged"] < info["examined"] // 4
    _assert_same(_whole(pkg, q, r, kn), want, f"whole edges kn={kn}")
    ix.close()


# ---- (c) the longest lists ----------------------------------------------------------------------------------------
def test_kn_256(pkg):
    k, m, n, kn = 32, 64, 140000, 256
    assert pkg.plan_topk_mfma(k, m, n, kn, bf16=True)["filtered"] == 1
    q = _pts(pkg, 51, m, k)
    r = _pts(pkg, 52, n, k)
    ix = pkg.Index(_dev(pkg, r), topk_mfma=True)
    got, info = _search(pkg, ix, _dev(pkg, q), kn)
    _assert_same(got, topk_oracle(q, r, kn), "kn=256")
    assert info["path"] == MFMA
    ix.close()


# ---- (d) ties at the kn-th distance -------------------------------------------------------------------------------
def test_ties_at_the_kth_distance(pkg):
    k, m, n, kn = 32, 64, 70001, 100
    p = pkg.plan_topk_mfma(k, m, n, kn, bf16=True)
    assert p["filtered"] == 1 and p["stride"] >= 2
    q = _pts(pkg, 61, m, k)
    r = _pts(pkg, 62, n, k)
    r[1000:1300] = q[0]                                  # 300 copies of query 0 straddle its 100th: the lowest indices win
    far = q[1].copy()
    far[0] = far[0] + np.float32(0.5) if far[0] < 0.5 else far[0] - np.float32(0.5)
    r[5000:5150] = far                                   # query 1: 150 refs at one distance, nearer than all others
    r = _as_searched(pkg, r, True)                       # (the moved coordinate rounded to bf16)
    want = topk_oracle(q, r, kn)
    assert want[0][0].tolist() == list(range(1000, 1100))
    inrun = (want[0][1] >= 5000) & (want[0][1] < 5150)
    assert 0 < inrun.sum() < 150 and inrun[-1]           # the run straddles query 1's kn-th distance
    ix = pkg.Index(_dev(pkg, r), topk_mfma=True)
    got, info = _search(pkg, ix, _dev(pkg, q), kn)
    assert info["path"] == MFMA
    assert not got[1][0].any()
    _assert_same(got, want, "ties")
    ix.close()


# ---- (e) a sample that says nothing about the other refs ----------------------------------------------------------
def test_unrepresentative_sample(pkg):
    k, m, n, kn = 32, 64, 20000, 10
    p = pkg.plan_topk_mfma(k, m, n, kn, bf16=True)
    assert p["filtered"] == 1 and p["stride"] >= 2
    q = _pts(pkg, 81, m, k)
    r = _pts(pkg, 82, n, k)
    sampled = (np.arange(n) // 32) % p["stride"] == 0
    r[sampled] += np.float32(8)                          # all sampled blocks far; the true neighbours in unsampled ones
    r = _as_searched(pkg, r, True)                       # (8 + x keeps five fraction bits: round once more)
    ix = pkg.Index(_dev(pkg, r), topk_mfma=True)
    got, info = _search(pkg, ix, _dev(pkg, q), kn)
    _assert_same(got, topk_oracle(q, r, kn), "sample far")
    assert info["path"] == MFMA and not np.any(sampled[got[0]])
    ix.close()


# ---- (f) the fall-backs and void queries --------------------------------------------------------------------------
def test_fallbacks_and_void_queries(pkg):
    k, m, n, kn = 32, 72, 6000, 10
    q = _pts(pkg, 101, m, k)
    r = _pts(pkg, 102, n, k)
    q[5, 3] = np.nan
    want = topk_oracle(q, r, kn)
    assert np.all(want[0][5] == -1)
    ix = pkg.Index(_dev(pkg, r), topk_mfma=True)
    got, info = _search(pkg, ix, _dev(pkg, q), kn)
    _assert_same(got, want, "void query")
    assert info["path"] == MFMA and info["filled"] == 1, info
    assert _nblk(n) <= info["flagged"] < m * _nblk(n), info          # one filled row; the rest filtered
    ref = pkg.Index(_dev(pkg, r), path="exact")
    assert torch.equal(ref.search_topk_keys(_dev(pkg, q), kn), ix.search_topk_keys(_dev(pkg, q), kn))   # K6's keys
    ref.close()
    got, info = _search(pkg, ix, _dev(pkg, q[:63]), kn)  # below the filter's query floor
    _assert_same(got, (want[0][:63], want[1][:63]), "63 queries")
    assert info == {"path": EXACT, "flagged": 0, "examined": 0, "filled": 0} and ix.stats()["path"] == EXACT
    ix.close()
    ix = pkg.Index(_dev(pkg, r[:3000]), topk_mfma=True)  # too few refs for a sample with stride 2
    assert pkg.plan_topk_mfma(k, m, 3000, kn, bf16=True)["filtered"] == 0
    got, info = _search(pkg, ix, _dev(pkg, q), kn)
    _assert_same(got, topk_oracle(q, r[:3000], kn), "small n")
    assert info["path"] == EXACT
    ix.close()
    r[77, 2] = np.inf                                    # refs_bad
    ix = pkg.Index(_dev(pkg, r), topk_mfma=True)
    got, info = _search(pkg, ix, _dev(pkg, q), kn)
    _assert_same(got, topk_oracle(q, r, kn), "inf ref")
    assert info["path"] == EXACT and ix.stats()["path"] == EXACT
    ix.close()
