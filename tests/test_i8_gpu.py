"""GPU tests of int8 points: the operand lane map of v_mfma_i32_16x16x64_i8 (selftest mode 6), 1-NN through the int8 filter
(both record forms) and through the exact kernels, the extreme values, ties, top-K, range search, the whole calls, the
resident index's lifecycle, the same-dtype rule and the agreement with a bf16 index built from the same values.  Every comparison is exact: indices equal
and distance bits equal to the V0 oracle on the values widened to fp32."""
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
I8 = 3


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _i8(seed, *shape, lo=-128, hi=128):
    """uniform over lo .. hi - 1"""
    return np.random.default_rng(seed).integers(lo, hi, shape).astype(np.int8)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _oracle(orc, q, r):
    return orc.v0_search(q.astype(np.float32), r.astype(np.float32))


def _search(pkg, q, r, **kw):
    """(idx, dist, stats) of one Index.search on the device"""
    ix = pkg.Index(_dev(r), **kw)
    idx, dist = ix.search(_dev(q), return_distances=True)
    torch.cuda.synchronize()
    st = ix.stats()
    ix.close()
    return idx.cpu().numpy(), dist.cpu().numpy(), st


def _same(got_idx, got_dist, want_idx, want_dist, what=""):
    assert np.array_equal(got_idx, want_idx), (what, np.flatnonzero(got_idx != want_idx)[:8])
    assert np.array_equal(_bits(got_dist), _bits(want_dist)), what


def _depth(pkg, k, m, n):
    return pkg.plan_filter(k, m, n, bf16=I8)["kt"]


# ---- the operand lane map ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kt", [64, 128, 256])
def test_i8_mfma_lane_map(pkg, kt):
    """Selftest mode 6 against integer arithmetic, exactly: asymmetric full-range operands (a and b are different draws,
    -128 and 127 among them), a seed per ref row.  A wrong A / B map or k order shows as gross mismatches."""
    for seed in (1, 2):
        rng = np.random.default_rng(seed * 100 + kt)
        a = rng.integers(-128, 128, (32, kt)).astype(np.int8)
        b = rng.integers(-128, 128, (32, kt)).astype(np.int8)
        a[3, 5], a[17, kt - 1], b[0, 0], b[31, 40] = -128, 127, 127, -128
        a[9, :] = -128                                         # the largest products against ...
        b[6, :] = -128                                         # ... 2^22 at kt = 256
        b[7, :] = 127
        assert a.min() == -128 and a.max() == 127 and b.min() == -128 and b.max() == 127
        c0 = rng.integers(-100000, 100000, 32).astype(np.float32)
        out = pkg.selftest_mfma(a.astype(np.float32), b.astype(np.float32), c0, bf16=6)
        want = c0.astype(np.int64)[:, None] + a.astype(np.int64) @ b.astype(np.int64).T     # [ref i][query j]
        assert np.abs(want).max() < 2 ** 24
        assert np.array_equal(out.astype(np.int64), want), (kt, seed, int((out.astype(np.int64) != want).sum()))
    out1 = np.zeros((32, 32), np.float32)
    z = np.zeros((32, 96), np.float32)
    assert pkg.lib.nns_selftest_mfma(96, 6, z.ctypes.data, z.ctypes.data, z.ctypes.data, out1.ctypes.data) == INVALID
    assert pkg.lib.nns_selftest_mfma(64, 7, z.ctypes.data, z.ctypes.data, z.ctypes.data, out1.ctypes.data) == INVALID


# ---- 1-NN -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_ref", [False, True])
@pytest.mark.parametrize("m,n,k", [(64, 2048, 128), (130, 5003, 100), (200, 4097, 256), (64, 33, 32), (96, 3000, 129)])
def test_1nn_through_the_i8_filter(pkg, orc, m, n, k, per_ref):
    q = _i8(100 + k, m, k)
    r = _i8(200 + k, n, k)
    want = _oracle(orc, q, r)
    idx, dist, st = _search(pkg, q, r, path="mfma_perref" if per_ref else "auto")
    assert st["path"] == MFMA and st["k_tile"] == _depth(pkg, k, m, n) and st["filter_form"] == "i8"
    assert st["nonfinite"] == 0
    _same(idx, dist, *want, (m, n, k, per_ref))
    # k <= 256: V0's distance is the integer squared distance
    dint = ((q.astype(np.int64) - r.astype(np.int64)[want[0]]) ** 2).sum(1)
    assert np.array_equal(dist.astype(np.int64), dint)


def test_extremes(pkg, orc):
    m, n, k = 96, 3000, 256
    r0 = _i8(2, n, k)

    def run(q, r, what):
        idx, dist, st = _search(pkg, q, r)
        assert st["path"] == MFMA and st["filter_form"] == "i8" and st["nonfinite"] == 0, (what, st)
        _same(idx, dist, *_oracle(orc, q, r), what)
        return idx, dist

    qlo = np.full((m, k), -128, np.int8)
    idx, dist = run(qlo, np.full((n, k), 127, np.int8), "all -128 against all 127")
    assert (dist == 16646400.0).all() and (idx == 0).all()                    # the largest distance; every ref ties
    idx, dist = run(qlo, np.full((n, k), -128, np.int8), "all -128 against all -128")
    assert (dist == 0.0).all() and (idx == 0).all()                           # the largest products, x.y = 2^22
    idx, dist = run(np.full((m, k), 127, np.int8), np.full((n, k), -128, np.int8), "all 127 against all -128")
    assert (dist == 16646400.0).all()
    r = r0.copy()                                                             # mixed: extreme refs among random ones,
    r[5] = 127                                                                # one ref equal to a query
    r[6] = -128
    q = _i8(3, m, k)
    q[0] = -128
    q[1] = 127
    q[9] = r[1234]
    idx, dist = run(q, r, "extreme rows among random ones")
    assert idx[0] == 6 and idx[1] == 5 and idx[9] == 1234 and dist[0] == 0 and dist[1] == 0 and dist[9] == 0


def test_ties_the_lowest_index_wins(pkg, orc):
    m, n, k = 128, 4096, 32
    rng = np.random.default_rng(7)
    q = rng.integers(0, 2, (m, k)).astype(np.int8)
    r = rng.integers(0, 2, (n, k)).astype(np.int8)
    d = v0_all(q.astype(np.float32), r.astype(np.float32))
    tied = ((d == d.min(axis=1, keepdims=True)).sum(axis=1) >= 2).sum()
    assert tied >= 32, tied
    idx, dist, st = _search(pkg, q, r)
    assert st["path"] == MFMA and st["filter_form"] == "i8"
    assert st["multi_candidate"] + st["ambiguous"] > 0, st
    _same(idx, dist, *_oracle(orc, q, r))
    # exact duplicates of a query at two indices: the lower wins
    m, n, k = 96, 3000, 64
    qd, rd = _i8(11, m, k), _i8(12, n, k)
    rd[2500] = rd[40]
    qd[9] = rd[40]
    rd[1200] = rd[1999]
    qd[10] = rd[1999]
    idx, dist, st = _search(pkg, qd, rd)
    assert st["path"] == MFMA and idx[9] == 40 and idx[10] == 1200 and dist[9] == 0 and dist[10] == 0
    _same(idx, dist, *_oracle(orc, qd, rd), "duplicates")


@pytest.mark.parametrize("m,n,k", [(5, 1000, 3), (70, 1500, 7), (40, 2000, 128), (64, 600, 300)])
def test_1nn_on_the_exact_path(pkg, orc, m, n, k):
    q = _i8(300 + k, m, k)
    r = _i8(400 + k, n, k)
    idx, dist, st = _search(pkg, q, r)
    assert st["path"] == EXACT and st["filter_form"] == (None if k < 32 or k > 256 else "i8") and st["nonfinite"] == 0
    _same(idx, dist, *_oracle(orc, q, r), (m, n, k))
    if 32 <= k <= 256:   # and forced onto the exact kernels at a filter depth
        idx, dist, st = _search(pkg, _i8(500 + k, 70, k), r, path="exact")
        assert st["path"] == EXACT
        _same(idx, dist, *_oracle(orc, _i8(500 + k, 70, k), r), "forced exact")
    if k > 256:   # no tile that deep for int8 points
        with pytest.raises(pkg.NNSError) as e:
            pkg.Index(_dev(r), path="mfma")
        assert e.value.status == UNSUPPORTED


# ---- top-K and range search ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(3, 70, 3000), (64, 33, 5003)], ids=["k3", "k64"])
def tr_case(request):
    """(q, r, V0 distances [m][n], stable order of every row) of one shape, computed once"""
    k, m, n = request.param
    q, r = _i8(500 + k, m, k), _i8(600 + k, n, k)
    r[n // 2] = r[11]                                   # a tie inside every query's list
    d = v0_all(q.astype(np.float32), r.astype(np.float32))
    return q, r, d, np.argsort(d, axis=1, kind="stable")


def test_topk_keys_equal_the_stable_sorted_oracle(pkg, tr_case):
    q, r, d, order = tr_case
    ix = pkg.Index(_dev(r))
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
    ix = pkg.Index(_dev(r))
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
    q, r = _i8(71, m, k), _i8(72, n, k)
    want = _oracle(orc, q, r)
    idx, dist = pkg.search_i8(q, r, return_distances=True)
    _same(idx, dist, *want, "auto")
    d = v0_all(q.astype(np.float32), r.astype(np.float32))
    order = np.argsort(d, axis=1, kind="stable")[:, :7]
    idx, dist = pkg.search_topk_i8(q, r, 7, return_distances=True)
    assert np.array_equal(idx, order) and np.array_equal(_bits(dist), _bits(np.take_along_axis(d, order, 1)))
    radius2 = float(np.sort(d, axis=None)[10 * m])
    wl, wi, wd = range_oracle(q.astype(np.float32), r.astype(np.float32), radius2)
    lims, idx, dist = pkg.search_range_i8(q, r, radius2, return_distances=True)
    assert np.array_equal(lims, wl) and np.array_equal(idx, wi) and np.array_equal(_bits(dist), _bits(wd))
    with pytest.raises(ValueError):
        pkg.search_i8(q.astype(np.float32), r)


# ---- the resident index's lifecycle ---------------------------------------------------------------------------------
def test_resident_index_lifecycle(pkg, orc):
    """test_f16_gpu.lifecycle_common for int8 points (index_base, a caller's stream, search_indices, changing m, shard
    merges, refresh), then a refresh to refs that hold rows of all -128 and all 127: the filter keeps running (no int8
    value is out of its range) and finds them."""
    m, n, k = 130, 5003, 100
    q, r, r_new = _i8(91, m, k), _i8(92, n, k), _i8(94, n, k)
    ix, rd, qd, base = lifecycle_common(pkg, orc, q, r, _i8(93, 700, k), r_new, "i8", I8)
    r_ext, q_ext = r_new.copy(), q.copy()
    r_ext[5], r_ext[4000] = -128, 127
    q_ext[0], q_ext[1] = -128, 127
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
    q, r = _i8(81, m, k), _i8(82, n, k)
    ix = pkg.Index(_dev(r))
    keys = torch.empty(m, dtype=torch.int64, device=DEV)
    q16 = _dev(q.astype(np.float16))
    with pytest.raises(ValueError):
        ix.search(q16)
    L = pkg.lib
    assert L.nns_index_search_f16(ix._h, m, q16.data_ptr(), keys.data_ptr(), None) == INVALID
    assert L.nns_index_search_bf16(ix._h, m, q16.data_ptr(), keys.data_ptr(), None) == INVALID
    assert L.nns_index_search(ix._h, m, q16.data_ptr(), keys.data_ptr(), None) == INVALID
    qd = _dev(q)
    assert L.nns_index_search_i8(ix._h, m, qd.data_ptr(), keys.data_ptr(), None) == 0
    torch.cuda.synchronize()
    ix.close()
    for other in (torch.float16, torch.bfloat16, torch.float32):       # and the reverse
        ixo = pkg.Index(_dev(r.astype(np.float32)).to(other))
        with pytest.raises(ValueError):
            ixo.search(qd)
        assert L.nns_index_search_i8(ixo._h, m, qd.data_ptr(), keys.data_ptr(), None) == INVALID
        ixo.close()


# ---- against a bf16 index on the same values ------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,k", [(200, 4097, 256), (130, 5003, 100)])
def test_keys_equal_a_bf16_index_on_the_same_values(pkg, m, n, k):
    q, r = _i8(900 + k, m, k), _i8(950 + k, n, k)
    ix8 = pkg.Index(_dev(r))
    k8 = ix8.search_keys(_dev(q)).cpu().numpy()
    ix8.close()
    rb = _dev(r.astype(np.float32)).to(torch.bfloat16)           # every int8 value is exact in bf16
    qb = _dev(q.astype(np.float32)).to(torch.bfloat16)
    assert torch.equal(rb.to(torch.float32).cpu(), torch.from_numpy(r.astype(np.float32)))
    ixb = pkg.Index(rb)
    kb = ixb.search_keys(qb).cpu().numpy()
    ixb.close()
    assert np.array_equal(k8, kb)
