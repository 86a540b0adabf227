"""GPU tests of uint8 points: 1-NN through the int8 filter on K2's biased image and through the exact kernels, rows of all 0
and all 255, planted duplicates, bit-equal keys against an int8 index on the values minus 128, top-K, range search, the
whole calls, the resident index's lifecycle and the same-dtype rule.  Every comparison is exact: indices equal and
distance bits equal to the V0 oracle on the values widened to fp32."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_f16_gpu import lifecycle_common  # noqa: E402
from test_range_cpu import range_oracle, v0_all  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
EXACT, MFMA = 1, 2
INVALID, UNSUPPORTED = 1, 5
U8 = 5


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _u8(seed, *shape):
    """uniform over 0 .. 255"""
    return np.random.default_rng(seed).integers(0, 256, shape).astype(np.uint8)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _biased(a):
    """the int8 values a - 128"""
    return (a.astype(np.int16) - 128).astype(np.int8)


def _oracle(orc, q, r):
    return orc.v0_search(q.astype(np.float32), r.astype(np.float32))


def _search(pkg, q, r, **kw):
    """(idx, dist, keys, stats) of one search of a uint8 index on the device"""
    ix = pkg.Index(_dev(r), points="u8", **kw)
    assert ix.u8 and not ix.b1 and ix.k == r.shape[1]
    qd = _dev(q)
    idx, dist = ix.search(qd, return_distances=True)
    keys = ix.search_keys(qd)
    torch.cuda.synchronize()
    st = ix.stats()
    ix.close()
    return idx.cpu().numpy(), dist.cpu().numpy(), keys.cpu().numpy(), st


def _i8_keys(pkg, q, r, **kw):
    """the keys of an int8 index on the biased refs, searched with the biased queries"""
    ix = pkg.Index(_dev(_biased(r)), **kw)
    keys = ix.search_keys(_dev(_biased(q)))
    torch.cuda.synchronize()
    ix.close()
    return keys.cpu().numpy()


def _same(got_idx, got_dist, want_idx, want_dist, what=""):
    assert np.array_equal(got_idx, want_idx), (what, np.flatnonzero(got_idx != want_idx)[:8])
    assert np.array_equal(_bits(got_dist), _bits(want_dist)), what


def _planted(seed, m, n, k):
    """random points with rows of all 0 and all 255 in refs and queries, and a duplicate of a query planted at a lower and
    a higher ref index (the lower wins)"""
    q, r = _u8(seed, m, k), _u8(seed + 1, n, k)
    r[7], r[n - 3] = 0, 255
    q[0], q[1] = 0, 255
    r[n - 100] = r[40]
    q[9] = r[40]
    r[n // 3] = r[n - 50]
    q[10] = r[n - 50]
    return q, r


# ---- 1-NN -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [32, 33, 64, 100, 128, 129, 256])
def test_1nn_through_the_i8_filter(pkg, orc, k):
    m, n = 130, 5003
    q, r = _planted(100 + k, m, n, k)
    want = _oracle(orc, q, r)
    idx, dist, keys, st = _search(pkg, q, r)
    assert st["path"] == MFMA and st["k_tile"] == 256 and st["filter_form"] == "i8" and st["nonfinite"] == 0, st
    _same(idx, dist, *want, k)
    assert idx[0] == 7 and idx[1] == n - 3 and idx[9] == 40 and idx[10] == n // 3
    assert dist[0] == 0 and dist[1] == 0 and dist[9] == 0 and dist[10] == 0
    # k <= 256: V0's distance is the integer squared distance
    dint = ((q.astype(np.int64) - r.astype(np.int64)[want[0]]) ** 2).sum(1)
    assert np.array_equal(dist.astype(np.int64), dint)
    # the bias identity: the same keys, bit for bit, as the int8 index on the values - 128
    assert np.array_equal(keys, _i8_keys(pkg, q, r)), k
    # and the other record form
    idx, dist, keys2, st = _search(pkg, q, r, path="mfma_perref")
    assert st["path"] == MFMA and np.array_equal(keys2, keys)


def test_extremes(pkg, orc):
    m, n, k = 96, 3000, 256
    for qv, rv, d in ((0, 255, 16646400.0), (255, 0, 16646400.0), (0, 0, 0.0), (255, 255, 0.0)):
        q, r = np.full((m, k), qv, np.uint8), np.full((n, k), rv, np.uint8)
        idx, dist, _, st = _search(pkg, q, r)
        assert st["path"] == MFMA and st["nonfinite"] == 0
        assert (dist == d).all() and (idx == 0).all(), (qv, rv)              # every ref ties: index 0


@pytest.mark.parametrize("m,n,k", [(5, 1000, 3), (70, 1500, 7), (40, 2000, 128), (64, 600, 300)])
def test_1nn_on_the_exact_path(pkg, orc, m, n, k):
    q, r = _planted(300 + k, m, n, k) if m > 10 else (_u8(300 + k, m, k), _u8(301 + k, n, k))
    idx, dist, keys, st = _search(pkg, q, r)
    assert st["path"] == EXACT and st["filter_form"] == (None if k < 32 or k > 256 else "i8") and st["nonfinite"] == 0
    _same(idx, dist, *_oracle(orc, q, r), (m, n, k))
    assert np.array_equal(keys, _i8_keys(pkg, q, r)), (m, n, k)
    if 32 <= k <= 256:   # and forced onto the exact kernels at a filter depth
        q70 = _u8(500 + k, 70, k)
        idx, dist, keys, st = _search(pkg, q70, r, path="exact")
        assert st["path"] == EXACT
        _same(idx, dist, *_oracle(orc, q70, r), "forced exact")
        assert np.array_equal(keys, _i8_keys(pkg, q70, r, path="exact"))
    if k > 256:   # no tile that deep for uint8 points
        with pytest.raises(pkg.NNSError) as e:
            pkg.Index(_dev(r), points="u8", path="mfma")
        assert e.value.status == UNSUPPORTED


# ---- top-K and range search ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(3, 70, 3000), (64, 33, 5003)], ids=["k3", "k64"])
def tr_case(request):
    """(q, r, V0 distances [m][n], stable order of every row) of one shape, computed once"""
    k, m, n = request.param
    q, r = _u8(500 + k, m, k), _u8(600 + k, n, k)
    r[n // 2] = r[11]                                   # a tie inside every query's list
    d = v0_all(q.astype(np.float32), r.astype(np.float32))
    return q, r, d, np.argsort(d, axis=1, kind="stable")


def test_topk_keys_equal_the_stable_sorted_oracle(pkg, tr_case):
    q, r, d, order = tr_case
    ix = pkg.Index(_dev(r), points="u8")
    qd = _dev(q)
    for kn in (1, 10, 100):
        keys = ix.search_topk_keys(qd, kn)
        torch.cuda.synchronize()
        sel = order[:, :kn]
        want = (np.take_along_axis(d, sel, 1).view(np.uint32).astype(np.uint64) << np.uint64(32)) | sel.astype(np.uint64)
        assert np.array_equal(keys.cpu().numpy().view(np.uint64), want), kn
        if kn == 1:
            assert np.array_equal(keys.cpu().numpy()[:, 0], ix.search_keys(qd).cpu().numpy())
    ix.close()


def test_range_search_matches_the_range_oracle(pkg, tr_case):
    q, r, d, order = tr_case
    m, n = d.shape
    ix = pkg.Index(_dev(r), points="u8")
    qd = _dev(q)
    r10 = float(np.sort(d, axis=None)[10 * m])          # about 10 hits per query
    for radius2 in (0.0, float("inf"), r10):
        want = range_oracle(q.astype(np.float32), r.astype(np.float32), radius2)
        if radius2 == r10:
            assert 5 * m <= want[0][-1] <= 20 * m
        lims, idx, dist = ix.search_range(qd, radius2, return_distances=True)
        torch.cuda.synchronize()
        assert np.array_equal(lims.cpu().numpy(), want[0]), radius2
        assert np.array_equal(idx.cpu().numpy(), want[1]), radius2
        assert np.array_equal(_bits(dist.cpu().numpy()), _bits(want[2])), radius2
    ix.close()


# ---- whole calls ----------------------------------------------------------------------------------------------------
def test_whole_calls(pkg, orc):
    m, n, k = 130, 5003, 100
    q, r = _planted(71, m, n, k)
    want = _oracle(orc, q, r)
    for path in ("auto", "mfma", "exact"):
        idx, dist = pkg.search_u8(q, r, return_distances=True, path=path)
        _same(idx, dist, *want, path)
    d = v0_all(q.astype(np.float32), r.astype(np.float32))
    order = np.argsort(d, axis=1, kind="stable")[:, :7]
    idx, dist = pkg.search_topk_u8(q, r, 7, return_distances=True)
    assert np.array_equal(idx, order) and np.array_equal(_bits(dist), _bits(np.take_along_axis(d, order, 1)))
    radius2 = float(np.sort(d, axis=None)[10 * m])
    wl, wi, wd = range_oracle(q.astype(np.float32), r.astype(np.float32), radius2)
    lims, idx, dist = pkg.search_range_u8(q, r, radius2, return_distances=True)
    assert np.array_equal(lims, wl) and np.array_equal(idx, wi) and np.array_equal(_bits(dist), _bits(wd))
    with pytest.raises(ValueError):
        pkg.search_u8(q.astype(np.int8), r)


# ---- the resident index's lifecycle ---------------------------------------------------------------------------------
class _U8Pkg:
    """The package with Index(...) bound to points="u8": lifecycle_common builds its indices from the tensors alone, and a
    torch.uint8 tensor alone means packed bits."""

    def __init__(self, pkg):
        self._pkg = pkg
        self.Index = functools.partial(pkg.Index, points="u8")

    def __getattr__(self, name):
        return getattr(self._pkg, name)


def test_resident_index_lifecycle(pkg, orc):
    """test_f16_gpu.lifecycle_common for uint8 points (index_base, a caller's stream, search_indices, changing m, shard
    merges, refresh), then a refresh to refs that hold rows of all 0 and all 255."""
    m, n, k = 130, 5003, 100
    q, r, r_new = _u8(91, m, k), _u8(92, n, k), _u8(94, n, k)
    ix, rd, qd, base = lifecycle_common(_U8Pkg(pkg), orc, q, r, _u8(93, 700, k), r_new, "i8", U8)
    assert ix.u8
    r_ext, q_ext = r_new.copy(), q.copy()
    r_ext[5], r_ext[4000] = 0, 255
    q_ext[0], q_ext[1] = 0, 255
    rd.copy_(torch.from_numpy(r_ext))
    ix.refresh()
    i, d = ix.search(_dev(q_ext), return_distances=True)
    torch.cuda.synchronize()
    i, d = i.cpu().numpy() - base, d.cpu().numpy()
    _same(i, d, *_oracle(orc, q_ext, r_ext), "extreme rows after refresh")
    assert i[0] == 5 and i[1] == 4000 and d[0] == 0 and d[1] == 0
    s = ix.stats()
    assert s["path"] == MFMA and s["nonfinite"] == 0 and s["filter_form"] == "i8", s
    ix.close()


def test_dtype_mismatch(pkg):
    m, n, k = 64, 512, 64
    q, r = _u8(81, m, k), _u8(82, n, k)
    ix = pkg.Index(_dev(r), points="u8")
    keys = torch.empty(m, dtype=torch.int64, device=DEV)
    qd = _dev(q)
    q8 = _dev(_biased(q))
    with pytest.raises(ValueError):
        ix.search(q8)
    L = pkg.lib
    for fn in (L.nns_index_search_i8, L.nns_index_search_f16, L.nns_index_search_bf16, L.nns_index_search, L.nns_index_search_b1):
        assert fn(ix._h, m, qd.data_ptr(), keys.data_ptr(), None) == INVALID
        assert b"uint8" in L.nns_last_error()
    assert L.nns_index_search_u8(ix._h, m, qd.data_ptr(), keys.data_ptr(), None) == 0
    torch.cuda.synchronize()
    ix.close()
    # and the reverse: a uint8 query set against every other index, packed-bit indices (the inferred meaning of uint8) included
    others = [pkg.Index(_dev(r.astype(np.float32)).to(t)) for t in (torch.float16, torch.bfloat16, torch.float32)]
    others += [pkg.Index(_dev(_biased(r))), pkg.Index(_dev(r))]
    assert others[-1].b1 and not others[-1].u8
    for ixo in others:
        assert L.nns_index_search_u8(ixo._h, m, qd.data_ptr(), keys.data_ptr(), None) == INVALID
        ixo.close()
    with pytest.raises(ValueError):
        pkg.Index(_dev(_biased(r)), points="u8")
    with pytest.raises(ValueError):
        pkg.Index(_dev(r), points="i8")
