"""GPU tests of binary points (packed bits, Hamming distance): 1-NN through K1b's Hamming scan (both load forms, the
staged and the plain kernel), every bit position, ties, alignment, top-K (K6), range search (K7) with its count / fill
contract, the whole calls, the agreement with an int8 index on the unpacked values, and the split API's manners.  Every
comparison is exact: indices equal and distance bits equal to the V0 oracles on the bits unpacked to fp32."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_range_cpu import range_oracle, v0_all  # noqa: E402
from test_topk_cpu import topk_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
EXACT = 1
OK, INVALID, UNSUPPORTED = 0, 1, 5
KEY_NONE = 0xFFFFFFFFFFFFFFFF


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rand(seed, n, k):
    """n random points of k bits, unpacked (uint8 0 / 1)"""
    return np.random.default_rng(seed).integers(0, 2, (n, k)).astype(np.uint8)


def _f(a):
    return a.astype(np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(got_idx, got_dist, want_idx, want_dist, what=""):
    assert np.array_equal(got_idx, want_idx), (what, np.flatnonzero(got_idx != want_idx)[:8])
    assert np.array_equal(_bits(got_dist), _bits(want_dist)), what


def _keys_of(d, sel, base=0):
    """packed keys of the entries sel [m][kn] of the distance matrix d (-1: NNS_KEY_NONE)"""
    dv = np.take_along_axis(d, np.maximum(sel, 0), 1)
    keys = (dv.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (sel + base).astype(np.uint64)
    return np.where(sel < 0, np.uint64(KEY_NONE), keys)


def _search(pkg, q, r, **kw):
    """(idx, dist, stats) of one Index.search of the packed points on the device"""
    ix = pkg.Index(_dev(pkg.pack_bits(r)), **kw)
    idx, dist = ix.search(_dev(pkg.pack_bits(q)), return_distances=True)
    torch.cuda.synchronize()
    st = ix.stats()
    ix.close()
    return idx.cpu().numpy(), dist.cpu().numpy(), st


# ---- 1-NN -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,k", [(5, 1000, 32), (70, 1500, 96), (130, 2999, 128), (64, 33, 160), (130, 5003, 256),
                                   (40, 2000, 1056), (3, 70001, 2048), (1, 4097, 256)])
def test_1nn_grid(pkg, orc, m, n, k):
    """One word, odd word counts, both VEC forms (k / 32 % 4), a long row, m and n tails, several grid-stride rounds, few
    queries."""
    q, r = _rand(100 + k + m, m, k), _rand(200 + k + m, n, k)
    want = orc.v0_search(_f(q), _f(r))
    idx, dist, st = _search(pkg, q, r)
    assert st["path"] == EXACT and st["nonfinite"] == 0 and st["filter_form"] is None, st
    _same(idx, dist, *want, (m, n, k))
    ham = (q != r[want[0]]).sum(axis=1)
    assert np.array_equal(dist, ham.astype(np.float32))      # the distance is the Hamming distance
    # the whole call gives the same answer
    widx, wdist = pkg.search_b1(pkg.pack_bits(q), pkg.pack_bits(r), return_distances=True)
    _same(widx, wdist, *want, ("whole call", m, n, k))


def test_every_bit_position_counts(pkg, orc):
    m, n, k = 70, 3000, 256
    q, r = _rand(1, m, k), _rand(2, n, k)
    for i, bit in enumerate((0, 31, 32, k - 1)):         # refs equal to query i but for one flipped bit
        r[100 + 500 * i] = q[i]
        r[100 + 500 * i, bit] ^= 1
    r[2900] = 1 - q[9]                                   # the complement of query 9 ...
    q[10] = q[9]                                         # ... and of query 10
    r[n - 1] = q[20]                                     # an exact duplicate at the last ref ...
    r[1700] = q[20]                                      # ... and the same at a lower index: the lower wins
    r[n - 2] = q[21]                                     # and one at the second to last ref alone
    d = v0_all(_f(q), _f(r))
    assert (d[9, 2900], d[10, 2900]) == (k, k)
    want = orc.v0_search(_f(q), _f(r))
    idx, dist, _ = _search(pkg, q, r)
    _same(idx, dist, *want)
    assert idx[:4].tolist() == [100, 600, 1100, 1600] and (dist[:4] == 1.0).all()
    assert idx[20] == 1700 and dist[20] == 0.0 and idx[21] == n - 2 and dist[21] == 0.0
    # the complement is the farthest ref: the last entry of query 9's full list, at distance k
    ti, td = pkg.search_topk_b1(pkg.pack_bits(q[9:10]), pkg.pack_bits(r[2800:]), 200, return_distances=True)
    assert ti[0, -1] == 100 and td[0, -1] == float(k)
    # all-zero against all-one rows
    idx, dist, _ = _search(pkg, np.zeros((3, k), np.uint8), np.ones((40, k), np.uint8))
    assert (idx == 0).all() and (dist == float(k)).all()


def test_ties_the_lowest_index_wins(pkg, orc):
    m, n, k = 128, 4096, 32
    rng = np.random.default_rng(7)
    q = rng.integers(0, 2, (m, k)).astype(np.uint8)
    r = rng.integers(0, 2, (n, k)).astype(np.uint8)
    d = v0_all(_f(q), _f(r))
    tied = ((d == d.min(axis=1, keepdims=True)).sum(axis=1) >= 2).sum()
    assert tied >= 32, tied
    idx, dist, _ = _search(pkg, q, r)
    _same(idx, dist, *orc.v0_search(_f(q), _f(r)))


def test_alignment(pkg, orc):
    m, n, k = 70, 1500, 128
    q, r = pkg.pack_bits(_rand(31, m, k)), pkg.pack_bits(_rand(32, n, k))
    want = orc.v0_search(_f(np.unpackbits(q, axis=1, bitorder="little")), _f(np.unpackbits(r, axis=1, bitorder="little")))

    def at(a, off):
        """a's rows in a flat device buffer whose data starts `off` bytes behind a 256-byte aligned address"""
        flat = torch.zeros(a.size + 512, dtype=torch.uint8, device=DEV)
        start = (-flat.data_ptr()) % 256 + off
        view = flat[start:start + a.size].view(a.shape[0], a.shape[1])
        view.copy_(torch.from_numpy(a))
        assert view.data_ptr() % 256 == off and view.is_contiguous()
        return view

    results = []
    for off in (0, 4):     # 16-byte aligned rows (dwordx4 loads, the staged kernel) and 4-aligned only (one word per step)
        rd, qd = at(r, off), at(q, off)
        ix = pkg.Index(rd)
        idx, dist = ix.search(qd, return_distances=True)
        tk = ix.search_topk_keys(qd, 10)
        lims, ridx = ix.search_range(qd, 50.0)
        torch.cuda.synchronize()
        _same(idx.cpu().numpy(), dist.cpu().numpy(), *want, off)
        results.append((tk.cpu().numpy(), lims.cpu().numpy(), ridx.cpu().numpy()))
        ix.close()
    for a, b in zip(*results):
        assert np.array_equal(a, b)
    assert results[0][1][-1] > 0
    # one byte off: refused on both sides, in Python and by the library
    r1, q1 = at(r, 1), at(q, 1)
    with pytest.raises(ValueError):
        pkg.Index(r1)
    h = ctypes.c_void_p()
    assert pkg.lib.nns_index_create_b1(ctypes.byref(h), 0, k, n, r1.data_ptr(), 0, 0, None) == INVALID and not h
    ix = pkg.Index(at(r, 0))
    keys = torch.empty((m, 2), dtype=torch.int64, device=DEV)
    lims = torch.empty(m + 1, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        ix.search(q1)
    assert pkg.lib.nns_index_search_b1(ix._h, m, q1.data_ptr(), keys.data_ptr(), None) == INVALID
    assert pkg.lib.nns_index_search_topk(ix._h, m, q1.data_ptr(), 2, keys.data_ptr(), None) == INVALID
    assert pkg.lib.nns_index_range_count(ix._h, m, q1.data_ptr(), 1.0, lims.data_ptr(), None) == INVALID
    ix.close()
    with pytest.raises(ValueError):
        pkg.Index(_dev(np.zeros((8, 6), np.uint8)))       # not whole words


# ---- top-K ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(64, 33, 5003), (96, 70, 3000)], ids=["k64", "k96"])
def tk_case(request):
    """(q, r unpacked, V0 distances [m][n], topk_oracle at kn = 256) of one shape, computed once"""
    k, m, n = request.param
    q, r = _rand(500 + k, m, k), _rand(600 + k, n, k)
    return q, r, v0_all(_f(q), _f(r)), topk_oracle(_f(q), _f(r), 256)


def test_topk_keys_equal_the_oracle(pkg, tk_case):
    q, r, d, (oi, od) = tk_case
    ix = pkg.Index(_dev(pkg.pack_bits(r)))
    qd = _dev(pkg.pack_bits(q))
    for kn in (1, 10, 100, 256):
        keys = ix.search_topk_keys(qd, kn)
        idx, dist = ix.search_topk(qd, kn, return_distances=True)
        torch.cuda.synchronize()
        assert np.array_equal(keys.cpu().numpy().view(np.uint64), _keys_of(d, oi[:, :kn].astype(np.int64))), kn
        assert np.array_equal(idx.cpu().numpy(), oi[:, :kn]) and np.array_equal(_bits(dist.cpu().numpy()), _bits(od[:, :kn])), kn
        if kn == 1:
            assert np.array_equal(keys.cpu().numpy()[:, 0], ix.search_keys(qd).cpu().numpy())
    ix.close()
    # the whole call, one shard and three
    for shards in (1, 3):
        idx, dist = pkg.search_topk_b1(pkg.pack_bits(q), pkg.pack_bits(r), 10, return_distances=True, shards=shards)
        assert np.array_equal(idx, oi[:, :10]) and np.array_equal(_bits(dist), _bits(od[:, :10])), shards


def test_topk_short_rows_and_repeated_flushes(pkg):
    k = 64
    q, r = _rand(41, 33, k), _rand(42, 33, k)
    oi, od = topk_oracle(_f(q), _f(r), 100)
    assert (oi[:, 33:] == -1).all() and np.isinf(od[:, 33:]).all()
    idx, dist = pkg.search_topk_b1(pkg.pack_bits(q), pkg.pack_bits(r), 100, return_distances=True)
    assert np.array_equal(idx, oi) and np.array_equal(_bits(dist), _bits(od))
    # refs sorted by descending distance to query 0: every round brings keys below its threshold, the queue flushes
    # again and again
    n = 5003
    r = _rand(43, n, k)
    order = np.argsort(-v0_all(_f(q[:1]), _f(r))[0], kind="stable")
    r = r[order]
    assert (np.diff(v0_all(_f(q[:1]), _f(r))[0]) <= 0).all()
    for kn in (10, 256):
        oi, od = topk_oracle(_f(q), _f(r), kn)
        idx, dist = pkg.search_topk_b1(pkg.pack_bits(q), pkg.pack_bits(r), kn, return_distances=True)
        assert np.array_equal(idx, oi) and np.array_equal(_bits(dist), _bits(od)), kn


# ---- range search -----------------------------------------------------------------------------------------------
def test_range_radii_and_the_count_fill_contract(pkg):
    m, n, k = 70, 3000, 96
    q, r = _rand(51, m, k), _rand(52, n, k)
    r[1234] = q[3]                                        # a hit at distance 0
    r[2000] = q[3]
    d = v0_all(_f(q), _f(r))
    dd = float(np.sort(d, axis=None)[10 * m])              # an integer distance that occurs
    assert dd == int(dd) and (d == dd).any()
    ix = pkg.Index(_dev(pkg.pack_bits(r)))
    qd = _dev(pkg.pack_bits(q))
    got = {}
    radii = (0.0, 0.5, dd, float(np.nextafter(np.float32(dd), np.float32(0))), float(k), float("inf"))
    for radius2 in radii:
        want = range_oracle(_f(q), _f(r), radius2)
        lims, idx, dist = ix.search_range(qd, radius2, return_distances=True)
        torch.cuda.synchronize()
        got[radius2] = (lims.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy())
        assert np.array_equal(got[radius2][0], want[0]), radius2
        assert np.array_equal(got[radius2][1], want[1]), radius2
        assert np.array_equal(_bits(got[radius2][2]), _bits(want[2])), radius2
        # the whole call
        wl, wi, wd = pkg.search_range_b1(pkg.pack_bits(q), pkg.pack_bits(r), radius2, return_distances=True)
        assert np.array_equal(wl, want[0]) and np.array_equal(wi, want[1]) and np.array_equal(_bits(wd), _bits(want[2])), radius2
    assert got[0.0][0][-1] == 2 and np.array_equal(got[0.5][1], got[0.0][1])          # 0.5: the hits of 0
    assert got[radii[3]][0][-1] == (d < dd).sum() < got[dd][0][-1] == (d <= dd).sum()   # inclusive; just below: excluded
    assert got[float(k)][0][-1] == m * n == got[float("inf")][0][-1]                  # every ref
    # count, other searches in between, then the fill; a wrong radius or m on the fill; two runs, identical bytes
    lims = ix.range_count(qd, dd)
    ix.search_keys(qd)
    ix.search_topk_keys(qd, 10)
    L = pkg.lib
    total = int(lims[-1].item())
    idx = torch.empty(total, dtype=torch.int32, device=DEV)
    assert L.nns_index_range_fill(ix._h, m, qd.data_ptr(), dd + 1.0, lims.data_ptr(), idx.data_ptr(), None, None) == INVALID
    assert L.nns_index_range_fill(ix._h, m - 1, qd.data_ptr(), dd, lims.data_ptr(), idx.data_ptr(), None, None) == INVALID
    idx1, dist1 = ix.range_fill(qd, dd, lims, total=total, return_distances=True)
    lims2 = ix.range_count(qd, dd)
    idx2, dist2 = ix.range_fill(qd, dd, lims2, return_distances=True)
    torch.cuda.synchronize()
    assert torch.equal(lims, lims2) and torch.equal(idx1, idx2) and torch.equal(dist1.view(torch.int32), dist2.view(torch.int32))
    assert np.array_equal(idx1.cpu().numpy(), got[dd][1]) and np.array_equal(_bits(dist1.cpu().numpy()), _bits(got[dd][2]))
    assert ix.range_info()["path"] == EXACT and ix.topk_info()["path"] in (0, EXACT)
    ix.close()


def test_range_over_several_chunks(pkg):
    m, n, k = 600, 70001, 32
    q, r = _rand(61, m, k), _rand(62, n, k)
    ms = 60                                                # the radius from a sample of the queries: the largest one
    counts = np.bincount(v0_all(_f(q[:ms]), _f(r)).astype(np.int64).ravel(), minlength=k + 1).cumsum()
    radius2 = float(np.flatnonzero(counts < 5 * ms)[-1])   # with fewer than 5 hits per query there
    want = range_oracle(_f(q), _f(r), radius2)
    assert 0 < want[0][-1] < 6 * m, (radius2, want[0][-1])
    assert pkg.plan_range(k, m, n, bf16=4)["chunks"] > 1
    ix = pkg.Index(_dev(pkg.pack_bits(r)))
    lims, idx, dist = ix.search_range(_dev(pkg.pack_bits(q)), radius2, return_distances=True)
    torch.cuda.synchronize()
    ix.close()
    assert np.array_equal(lims.cpu().numpy(), want[0]) and np.array_equal(idx.cpu().numpy(), want[1])
    assert np.array_equal(_bits(dist.cpu().numpy()), _bits(want[2]))


# ---- against an int8 index on the same values ---------------------------------------------------------------------
@pytest.mark.parametrize("k", [64, 256])
def test_keys_equal_an_int8_index_on_the_unpacked_values(pkg, k):
    m, n = 130, 5003
    q, r = _rand(900 + k, m, k), _rand(950 + k, n, k)
    ix8 = pkg.Index(_dev(r.astype(np.int8)))
    q8 = _dev(q.astype(np.int8))
    ixb = pkg.Index(_dev(pkg.pack_bits(r)))
    qb = _dev(pkg.pack_bits(q))
    assert np.array_equal(ix8.search_keys(q8).cpu().numpy(), ixb.search_keys(qb).cpu().numpy())
    assert ix8.stats()["path"] == 2 and ixb.stats()["path"] == EXACT          # the int8 arm went through its MFMA filter
    assert np.array_equal(ix8.search_topk_keys(q8, 10).cpu().numpy(), ixb.search_topk_keys(qb, 10).cpu().numpy())
    radius2 = float(k // 2 - k // 16)                      # one (k = 64) or two (k = 256) standard deviations below the mean
    a, b = ix8.search_range(q8, radius2, return_distances=True), ixb.search_range(qb, radius2, return_distances=True)
    torch.cuda.synchronize()
    assert a[0][-1].item() > m
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
    ix8.close()
    ixb.close()


# ---- the split API's manners --------------------------------------------------------------------------------------
def test_split_api_manners(pkg, orc):
    m, n, k = 70, 3000, 96
    q, r = _rand(71, m, k), _rand(72, n, k)
    want = orc.v0_search(_f(q), _f(r))
    d = v0_all(_f(q), _f(r))
    base = 10 ** 6
    rd, qd = _dev(pkg.pack_bits(r)), _dev(pkg.pack_bits(q))
    before = torch.cuda.current_device()
    ix = pkg.Index(rd, index_base=base, profile=True)
    assert ix.b1 and ix.k == k and ix.n == n
    # a caller stream; index_base in 1-NN, top-K and range
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        keys = ix.search_keys(qd, stream=st)
        tk = ix.search_topk_keys(qd, 5, stream=st)
        lims, ridx = ix.search_range(qd, 30.0, stream=st)
    st.synchronize()
    assert np.array_equal(keys.cpu().numpy().view(np.uint64), _keys_of(d, want[0][:, None].astype(np.int64), base)[:, 0])
    oi, _ = topk_oracle(_f(q), _f(r), 5)
    assert np.array_equal(tk.cpu().numpy().view(np.uint64), _keys_of(d, oi.astype(np.int64), base))
    wl, wi, _ = range_oracle(_f(q), _f(r), 30.0, index_base=base)
    assert np.array_equal(lims.cpu().numpy(), wl) and np.array_equal(ridx.cpu().numpy(), wi)
    idx = ix.search_indices(qd)
    torch.cuda.synchronize()
    assert np.array_equal(idx.cpu().numpy(), want[0] + base)
    s = ix.stats()
    assert s["path"] == EXACT and s["nonfinite"] == 0 and s["filter_form"] is None, s
    assert ix.near_ties().size == 0
    # refresh() after rewriting the refs in place
    r2 = _rand(73, n, k)
    rd.copy_(torch.from_numpy(pkg.pack_bits(r2)))
    ix.refresh()
    i2, d2 = ix.search(qd, return_distances=True)
    torch.cuda.synchronize()
    w2 = orc.v0_search(_f(q), _f(r2))
    _same(i2.cpu().numpy() - base, d2.cpu().numpy(), *w2, "after refresh")
    assert torch.cuda.current_device() == before
    ix.close()
    # what the index does not take surfaces the library's status
    for kw, status in ((dict(soa=True), UNSUPPORTED), (dict(range_mfma=True), UNSUPPORTED), (dict(topk_mfma=True), UNSUPPORTED),
                       (dict(path="mfma"), UNSUPPORTED), (dict(filter_bf16=True), INVALID), (dict(filter_f32=True), INVALID),
                       (dict(filter_split_eager=True), INVALID)):
        with pytest.raises(pkg.NNSError) as e:
            pkg.Index(_dev(np.zeros((96, 96), np.uint8)), **kw)
        assert e.value.status == status, kw


def test_dtype_mismatch(pkg):
    m, n, k = 64, 512, 64
    q, r = _rand(81, m, k), _rand(82, n, k)
    ix = pkg.Index(_dev(pkg.pack_bits(r)))
    keys = torch.empty(m, dtype=torch.int64, device=DEV)
    qb = _dev(pkg.pack_bits(q))
    q8 = _dev(q.astype(np.int8))
    with pytest.raises(ValueError):
        ix.search(q8)
    with pytest.raises(ValueError):
        ix.search(_dev(pkg.pack_bits(_rand(83, m, 96))))      # another width
    L = pkg.lib
    for fn in (L.nns_index_search, L.nns_index_search_bf16, L.nns_index_search_f16, L.nns_index_search_i8):
        assert fn(ix._h, m, qb.data_ptr(), keys.data_ptr(), None) == INVALID
    assert L.nns_index_search_b1(ix._h, m, qb.data_ptr(), keys.data_ptr(), None) == OK
    torch.cuda.synchronize()
    ix.close()
    others = [_dev(_f(r)).to(t) for t in (torch.float32, torch.bfloat16, torch.float16)] + [_dev(r.astype(np.int8))]
    for ro in others:                                         # and the reverse
        ixo = pkg.Index(ro)
        with pytest.raises(ValueError):
            ixo.search(qb)
        assert L.nns_index_search_b1(ixo._h, m, qb.data_ptr(), keys.data_ptr(), None) == INVALID
        ixo.close()
