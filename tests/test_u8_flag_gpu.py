"""GPU tests of the flag pass for uint8 points (NNS_RANGE_MFMA / NNS_TOPK_MFMA on a uint8 index: range_flag_u8_kernel on
v_mfma_i32_16x16x64_i8 over the biased int8 image, 32 <= k <= 256).  Lims, indices, keys and distance bits equal the numpy
oracles on the values widened to fp32, through the split API of a flagged index and the whole calls.  The threshold is
exact, so the sharpest check is on the flags themselves: a (query, 32-ref block) pair is flagged if and only if the block
holds a hit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_range_cpu import range_oracle, v0_all  # noqa: E402
from test_range_gpu import _assert_same, _radii  # noqa: E402
from test_topk_cpu import topk_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
INF = float("inf")
EXACT, MFMA = 1, 2
INVALID = 1
U8 = 5


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _u8(seed, *shape):
    return np.random.default_rng(seed).integers(0, 256, shape).astype(np.uint8)


def _f(a):
    return a.astype(np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(out):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _range(ix, qd, radius2):
    """((lims, idx, dist) on the host, range_info of the count) of one split-API range search."""
    out = ix.search_range(qd, radius2, return_distances=True)
    return _host(out), ix.range_info()


def _whole_range(pkg, q, r, radius2):
    return pkg.search_range_u8(q, r, radius2, return_distances=True, range_mfma=True)


def _keys_of(d, sel, base=0):
    """the packed keys of refs sel [m][kn] of the distance matrix d"""
    return (np.take_along_axis(d, sel, 1).view(np.uint32).astype(np.uint64) << np.uint64(32)) | (sel + base).astype(np.uint64)


def _blocks_with_a_hit(d, radius2):
    """the number of (query, 32-ref block) pairs that hold at least one ref within radius2"""
    m, n = d.shape
    nblk = -(-n // 32)
    dpad = np.full((m, nblk * 32), np.inf, np.float32)
    dpad[:, :n] = d
    return int((dpad.reshape(m, nblk, 32).min(axis=2) <= np.float32(radius2)).sum())


# ---- the range grid, and the flags' exactness -----------------------------------------------------------------------
@pytest.mark.parametrize("k", [32, 40, 64, 100, 128, 129, 200, 256])
def test_range_grid_and_exact_flags(pkg, k):
    m, n = 130, 2999
    q, r = _u8(10 + k, m, k), _u8(20 + k, n, k)
    r[100:140] = r[7]                                    # a run of equal distances for every query
    d = v0_all(_f(q), _f(r))
    radii = _radii(d, n)
    p = pkg.plan_range_mfma(k, m, n, bf16=U8)
    assert p["kt"] == 256 and p["layout"] == 3
    blocks = p["blocks_per_query"]
    ix = pkg.Index(_dev(r), points="u8", range_mfma=True)
    qd = _dev(q)
    for radius2 in radii:
        want = range_oracle(_f(q), _f(r), radius2)
        got, info = _range(ix, qd, radius2)
        _assert_same(got, want, f"split k={k} r2={radius2}")
        assert info["path"] == (EXACT if radius2 == INF else MFMA), (radius2, info)   # +INF takes K7
        assert info["hits"] == want[0][-1]
        if radius2 != INF:
            assert info["examined"] == m * blocks
            assert ix.stats()["path"] == MFMA
            # the exact threshold: flagged if and only if the block holds a hit
            assert info["flagged"] == _blocks_with_a_hit(d, radius2), (k, radius2, info)
        _assert_same(_whole_range(pkg, q, r, radius2), want, f"whole k={k} r2={radius2}")
    # a finite radius beyond every distance: every real ref of every query, no padded one
    got, info = _range(ix, qd, 1e9)
    assert info["path"] == MFMA and info["hits"] == m * n and info["flagged"] == m * -(-n // 32)
    _assert_same(got, range_oracle(_f(q), _f(r), 1e9), f"k={k} r2=1e9")
    assert np.array_equal(got[1].reshape(m, n), np.broadcast_to(np.arange(n, dtype=np.int32), (m, n)))
    ix.close()


# ---- several ring slots, splits and chunks; block edges --------------------------------------------------------------
@pytest.fixture(scope="module")
def edges():
    k, m, n = 32, 600, 70001                             # two query groups of 512; 69 flag words: two chunks
    q, r = _u8(41, m, k), _u8(42, n, k)
    spots = (0, 31, 32, n - 1, n - 9, 2047 * 32 + 5, 2048 * 32)
    for i, j in enumerate(spots):
        r[j] = q[7 * i]                                  # exact duplicates at block edges, the chunk edge, the last block
    return k, m, n, q, r, spots, v0_all(_f(q), _f(r))


def test_slots_splits_chunks_and_block_edges(pkg, edges):
    k, m, n, q, r, spots, d = edges
    p = pkg.plan_range_mfma(k, m, n, bf16=U8)
    assert p["grid_x"] == 2 and p["grid_y"] > 1
    assert -(-p["blocks_per_query"] // 32) == 69
    assert pkg.plan_topk_mfma(k, m, n, 1, bf16=U8)["chunks"] == 2          # (the evaluation's chunks are the selection's)
    radius2 = _radii(d, n)[1]                            # about 3 hits per query
    want = range_oracle(_f(q), _f(r), radius2)
    assert 2 * m < want[0][-1] < 6 * m
    ix = pkg.Index(_dev(r), points="u8", range_mfma=True)
    got, info = _range(ix, _dev(q), radius2)
    _assert_same(got, want, "edges")
    assert info["path"] == MFMA and info["flagged"] == _blocks_with_a_hit(d, radius2)
    for i, j in enumerate(spots):
        row = slice(got[0][7 * i], got[0][7 * i + 1])
        assert j in got[1][row].tolist() and got[2][row][got[1][row] == j] == 0.0, (i, j)
    _assert_same(_whole_range(pkg, q, r, radius2), want, "whole edges")
    ix.close()


# ---- the inclusive boundary ---------------------------------------------------------------------------------------------
def test_radius_is_inclusive_and_one_less_excluded(pkg):
    k, m, n = 40, 64, 5000
    q, r = _u8(51, m, k), _u8(52, n, k)
    d = v0_all(_f(q), _f(r))
    ix = pkg.Index(_dev(r), points="u8", range_mfma=True)
    qd = _dev(q)
    for i in (0, 7, 63):
        j = int(np.argsort(d[i], kind="stable")[50])
        radius2 = float(d[i, j])
        assert radius2 == int(radius2) and radius2 >= 1
        at, info = _range(ix, qd, radius2)
        assert info["path"] == MFMA and info["flagged"] == _blocks_with_a_hit(d, radius2)
        assert j in at[1][at[0][i]:at[0][i + 1]].tolist()                # a radius equal to a distance that occurs: in
        short, info = _range(ix, qd, radius2 - 1.0)
        assert info["path"] == MFMA and info["flagged"] == _blocks_with_a_hit(d, radius2 - 1.0)
        assert j not in short[1][short[0][i]:short[0][i + 1]].tolist()   # that distance minus 1: out
        _assert_same(at, range_oracle(_f(q), _f(r), radius2), "inclusive")
        _assert_same(short, range_oracle(_f(q), _f(r), radius2 - 1.0), "one less")
        # and a radius between two integers counts as the integer below it
        half, info = _range(ix, qd, radius2 - 0.5)
        _assert_same(half, short, "half")
    ix.close()


# ---- the fall-backs and the count / fill contract ---------------------------------------------------------------------
def test_63_queries_take_the_exact_kernels(pkg):
    k, m, n = 64, 63, 70001
    q, r = _u8(61, m, k), _u8(62, n, k)
    d = v0_all(_f(q), _f(r))
    radius2 = _radii(d, n)[1]
    ix = pkg.Index(_dev(r), points="u8", range_mfma=True, topk_mfma=True)
    got, info = _range(ix, _dev(q), radius2)
    _assert_same(got, range_oracle(_f(q), _f(r), radius2), "63 queries")
    assert info["path"] == EXACT and info["flagged"] == 0
    keys = ix.search_topk_keys(_dev(q), 10)
    torch.cuda.synchronize()
    assert ix.topk_info()["path"] == EXACT
    sel = np.argsort(d, axis=1, kind="stable")[:, :10]
    assert np.array_equal(keys.cpu().numpy().view(np.uint64), _keys_of(d, sel))
    ix.close()


def test_a_fill_must_match_its_count(pkg):
    k, m, n = 32, 80, 30000
    q, r = _u8(111, m, k), _u8(112, n, k)
    d = v0_all(_f(q), _f(r))
    radius2 = _radii(d, n)[2]
    want = range_oracle(_f(q), _f(r), radius2)
    qd, rd, q2 = _dev(q), _dev(r), _dev(_u8(113, 300, k))
    L = pkg.lib
    ix = pkg.Index(rd, points="u8", range_mfma=True, topk_mfma=True)
    ref_keys = ix.search_keys(q2).clone()
    lims = ix.range_count(qd, radius2)
    assert ix.range_info()["path"] == MFMA
    total = int(lims[-1].item())
    idx = torch.full((total,), -7, dtype=torch.int32, device=DEV)
    dist = torch.full((total,), -7.0, dtype=torch.float32, device=DEV)
    args = (lims.data_ptr(), idx.data_ptr(), dist.data_ptr(), None)
    assert L.nns_index_range_fill(ix._h, m, qd.data_ptr(), float(radius2) + 1.0, *args) == INVALID
    assert L.nns_index_range_fill(ix._h, m - 1, qd.data_ptr(), radius2, *args) == INVALID
    keys = ix.search_keys(q2)                            # a 1-NN and a top-K search in between are allowed
    tk = ix.search_topk_keys(q2, 3)
    assert ix.topk_info()["path"] in (EXACT, MFMA)
    ix.range_fill(qd, radius2, lims, idx=idx, dist=dist, return_distances=True)
    torch.cuda.synchronize()
    assert torch.equal(keys, ref_keys) and torch.equal(tk[:, 0], ref_keys)
    _assert_same(_host((lims, idx, dist)), want, "count, searches, fill")
    # another count ends what the first one's fill could use
    lims2 = ix.range_count(qd, float(radius2) + 1.0)
    torch.cuda.synchronize()
    assert L.nns_index_range_fill(ix._h, m, qd.data_ptr(), radius2, *args) == INVALID
    del lims2
    ix.close()


# ---- top-K through K6m --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def topk_case():
    k, m, n = 64, 130, 70001
    q, r = _u8(71, m, k), _u8(72, n, k)
    r[100:140] = r[7]                                    # a run of equal distances for every query
    d = v0_all(_f(q), _f(r))
    return k, m, n, q, r, d, np.argsort(d, axis=1, kind="stable")[:, :100]


@pytest.mark.parametrize("kn", [1, 10, 100])
def test_topk_keys_equal_the_oracle_and_k6(pkg, topk_case, kn):
    k, m, n, q, r, d, order = topk_case
    base = 10 ** 6
    p = pkg.plan_topk_mfma(k, m, n, kn, bf16=U8)
    assert p["filtered"] == 1 and p["kt"] == 256 and p["layout"] == 3
    rd, qd = _dev(r), _dev(q)
    ix = pkg.Index(rd, points="u8", index_base=base, topk_mfma=True)
    keys = ix.search_topk_keys(qd, kn)
    torch.cuda.synchronize()
    info = ix.topk_info()
    assert info["path"] == MFMA and info["examined"] == m * p["blocks_per_query"] and info["filled"] == 0, info
    assert 0 < info["flagged"] <= m * -(-n // 32)
    want = _keys_of(d, order[:, :kn], base)
    assert np.array_equal(keys.cpu().numpy().view(np.uint64), want), kn
    plain = pkg.Index(rd, points="u8", index_base=base)
    k6 = plain.search_topk_keys(qd, kn)
    torch.cuda.synchronize()
    assert plain.topk_info()["path"] != MFMA and torch.equal(keys, k6)    # (an unflagged index keeps no report: K6)
    plain.close()
    ix.close()
    idx, dist = pkg.search_topk_u8(q, r, kn, return_distances=True, topk_mfma=True)
    assert np.array_equal(idx, order[:, :kn]) and np.array_equal(_bits(dist), _bits(np.take_along_axis(d, order[:, :kn], 1)))


def test_topk_fall_backs_and_short_rows(pkg, topk_case):
    k, m, n, q, r, d, order = topk_case
    n3 = 3000                                            # too few refs for a sample: the stride is below 2
    assert pkg.plan_topk_mfma(k, m, n3, 10, bf16=U8)["filtered"] == 0 and pkg.plan_topk_mfma(k, m, n3, 10, bf16=U8)["stride"] < 2
    ix = pkg.Index(_dev(r[:n3]), points="u8", topk_mfma=True)
    keys = ix.search_topk_keys(_dev(q), 10)
    torch.cuda.synchronize()
    assert ix.topk_info()["path"] == EXACT
    d3 = d[:, :n3]
    assert np.array_equal(keys.cpu().numpy().view(np.uint64), _keys_of(d3, np.argsort(d3, axis=1, kind="stable")[:, :10]))
    ix.close()
    ix = pkg.Index(_dev(r[:5]), points="u8", topk_mfma=True)   # n = 5 < kn: the rows are padded
    keys = ix.search_topk_keys(_dev(q), 8)
    torch.cuda.synchronize()
    got = keys.cpu().numpy()
    d5 = d[:, :5]
    assert np.array_equal(got[:, :5].view(np.uint64), _keys_of(d5, np.argsort(d5, axis=1, kind="stable")))
    assert (got[:, 5:] == pkg.NNS_KEY_NONE).all()
    ix.close()


# ---- query batches --------------------------------------------------------------------------------------------------------
def test_two_query_batches(pkg):
    """2^20 queries x 70000 refs at k = 32 need 69 flag words per query: two batches under the 256 MiB cap.  The whole
    range result equals K7's on an unflagged index; queries around the batch boundary and at both ends are held against
    the oracles directly, for the range search and for top-2."""
    k, m, n, kn = 32, 1 << 20, 70000, 2
    p = pkg.plan_range_mfma(k, m, n, bf16=U8)
    pt = pkg.plan_topk_mfma(k, m, n, kn, bf16=U8)
    assert p["batches"] == 2 and pt["filtered"] == 1 and pt["batches"] == 2
    g = torch.Generator(device=DEV)
    g.manual_seed(15)
    qd = torch.randint(0, 256, (m, k), generator=g, device=DEV, dtype=torch.uint8)
    rd = torch.randint(0, 256, (n, k), generator=g, device=DEV, dtype=torch.uint8)
    ref = pkg.Index(rd, points="u8")
    _, d1 = ref.search(qd[:256].contiguous(), return_distances=True)
    radius2 = float(d1.median().item())                  # about one hit per query
    ix = pkg.Index(rd, points="u8", range_mfma=True, topk_mfma=True)
    got = ix.search_range(qd, radius2, return_distances=True)
    info = ix.range_info()
    assert info["path"] == MFMA and info["hits"] == int(got[0][-1].item()) > m // 8
    assert info["examined"] == m * p["blocks_per_query"] and 0 < info["flagged"] <= info["hits"]
    want = ref.search_range(qd, radius2, return_distances=True)
    assert ref.range_info()["path"] == EXACT
    torch.cuda.synchronize()
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    b = p["batch"]
    sel = [0, 1, b - 2, b - 1, b, b + 1, m - 2, m - 1]
    lims = got[0].cpu().numpy()
    idx, dist = got[1].cpu().numpy(), got[2].cpu().numpy()
    qs, rs = _f(qd[sel].cpu().numpy()), _f(rd.cpu().numpy())
    worc = range_oracle(qs, rs, radius2)
    got_i = np.concatenate([idx[lims[i]:lims[i + 1]] for i in sel])
    got_d = np.concatenate([dist[lims[i]:lims[i + 1]] for i in sel])
    got_l = np.concatenate([[0], np.cumsum([lims[i + 1] - lims[i] for i in sel])])
    _assert_same((got_l, got_i, got_d), worc, "batch boundary")
    keys = ix.search_topk_keys(qd, kn)
    tinfo = ix.topk_info()
    assert tinfo["path"] == MFMA and tinfo["examined"] == m * pt["blocks_per_query"] and tinfo["filled"] == 0
    ti, td = pkg.keys_topk_unpack(keys[sel].contiguous(), return_distances=True)
    torch.cuda.synchronize()
    wi, wd = topk_oracle(qs, rs, kn)
    assert np.array_equal(ti.cpu().numpy(), wi) and np.array_equal(_bits(td.cpu().numpy()), _bits(wd))
    ix.close()
    ref.close()
