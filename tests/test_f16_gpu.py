"""GPU tests of fp16 points (IEEE binary16): the f16 MFMA's error model behind tau mode 4, 1-NN through the f16 filter
(v_mfma_f32_16x16x32_f16 at KT = 128 / 256) and through the exact kernels, near ties, special values and the 32752 guard,
subnormal operands, top-K, range search, the whole calls, the resident index's lifecycle (index_base, caller streams,
changing m, shard merges, refresh and its stale-flag window) and the same-dtype rule.  Every comparison is exact: indices
equal and distance bits equal to the V0 oracle on the values widened to fp32 (numpy's float16 does the widening)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_parity import _bf16_model_cases  # noqa: E402
from test_range_cpu import range_oracle, v0_all  # noqa: E402
from test_topk_cpu import topk_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
EXACT, MFMA = 1, 2
INVALID, UNSUPPORTED = 1, 5
KEY_NONE = 0x7F80000000000000


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _u16(seed, *shape):
    """U[0, 1) rounded to fp16"""
    return np.random.default_rng(seed).random(shape, dtype=np.float32).astype(np.float16)


def _dev(a16):
    return torch.from_numpy(np.ascontiguousarray(a16)).to(DEV)


def _oracle(orc, q16, r16):
    return orc.v0_search(q16.astype(np.float32), r16.astype(np.float32))


def _search(pkg, q16, r16, **kw):
    """(idx, dist, stats) of one Index.search on the device"""
    ix = pkg.Index(_dev(r16), **kw)
    idx, dist = ix.search(_dev(q16), return_distances=True)
    torch.cuda.synchronize()
    st = ix.stats()
    ix.close()
    return idx.cpu().numpy(), dist.cpu().numpy(), st


def _same(got_idx, got_dist, want_idx, want_dist, what=""):
    assert np.array_equal(got_idx, want_idx), (what, np.flatnonzero(got_idx != want_idx)[:8])
    assert np.array_equal(_bits(got_dist), _bits(want_dist)), what


# ---- the error model: the f16 MFMA's accumulation, and subnormal operands ---------------------------------------------
def _f16_model_cases(rng, kt):
    """test_bf16_mfma_error_model's operand families (all inside binary16's range: |v| <= 2^13), plus the two subnormal
    families.  fp32 values; the test rounds them to fp16."""
    cases = list(_bf16_model_cases(rng, kt))
    u01 = lambda: rng.random((32, kt), dtype=np.float32)                       # noqa: E731
    # every operand a nonzero binary16 subnormal (U[0, 1) x 2^-14; asymmetric: a and b are different draws)
    sub = lambda v: np.clip(v, 2.0 ** -10, 1.0 - 2.0 ** -9).astype(np.float32) * np.float32(2.0 ** -14)   # noqa: E731
    cases.append(("all_subnormal", sub(u01()) * -1.0, sub(u01())))
    # unit-scale rows, every tenth element subnormal
    a, b = u01() * -2.0, u01()
    a[:, ::10] = -sub(u01()[:, ::10])
    b[:, 3::10] = sub(u01()[:, 3::10])
    cases.append(("tenth_subnormal", a, b))
    return cases


@pytest.mark.parametrize("kt", [128, 256])
def test_f16_mfma_error_model(pkg, kt):
    """The acceptance rule of test_bf16_mfma_error_model, unchanged, for v_mfma_f32_16x16x32_f16 (selftest mode 5, mode
    2's lane mapping) against fp64 on fp16-representable operands: the worst |hardware - fp64| of any output at most 1/4
    of the e3 bound of tau mode 4, and every element within 2 (kt + kt/16 + 2) u sum|terms|.  The two subnormal families
    are held to the same bounds: flushed subnormal operands would show as errors of the size of the dropped terms.  A
    wrong A / B lane map shows as O(1) errors (the operands are asymmetric)."""
    u = 2.0 ** -24
    worst, worst_sub = 0.0, 0.0
    for seed in (2, 3, 5, 8):
        rng = np.random.default_rng(seed * 1000 + kt + 16)
        for name, a32, b32 in _f16_model_cases(rng, kt):
            a = a32.astype(np.float16).astype(np.float32)
            b = b32.astype(np.float16).astype(np.float32)
            assert np.isfinite(a).all() and np.isfinite(b).all()
            if name == "all_subnormal":
                assert (np.abs(a) < 2.0 ** -14).all() and (a != 0).all() and (np.abs(b) < 2.0 ** -14).all() and (b != 0).all()
            a64, b64 = a.astype(np.float64), b.astype(np.float64)
            c0 = ((a64 / 2) ** 2).sum(1).astype(np.float32)           # the refs' squared norms (a = -2 y)
            out = pkg.selftest_mfma(a, b, c0, bf16=5)
            exact = c0.astype(np.float64)[:, None] + a64 @ b64.T
            err = np.abs(out.astype(np.float64) - exact)                # [ref i][query j]
            y2max = float(((a64 / 2) ** 2).sum(1).max())
            sub = "subnormal" in name
            for j in range(32):
                x2 = float((b64[j] ** 2).sum())
                c0t, c1t, _ = pkg.tau_consts(kt, x2, y2max, 4)
                e3 = c0t / (2.0 + c1t) / 1.001
                ratio = err[:, j].max() / e3
                if sub:
                    worst_sub = max(worst_sub, ratio)
                else:
                    worst = max(worst, ratio)
                assert ratio <= 0.25, (name, seed, kt, j, err[:, j].max(), e3)
            mag = np.abs(c0.astype(np.float64))[:, None] + np.abs(a64) @ np.abs(b64).T
            assert (err <= 2 * (kt + kt // 16 + 2) * u * mag).all(), (name, seed, kt)
            if name == "all_subnormal":
                # not flushed: the products are there (a flush gives exactly 0 where the exact sum is > 0)
                assert (out != 0).all() and np.all(np.abs(out.astype(np.float64) - exact) <= 1e-3 * np.abs(exact))
    print(f"f16 MFMA kt {kt}: worst error / e3 bound = {worst:.4f}; subnormal families: {worst_sub:.4f}")


# ---- 1-NN -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_ref", [False, True])
@pytest.mark.parametrize("m,n,k", [(64, 2048, 128), (130, 5003, 100), (200, 4097, 256), (64, 33, 32), (96, 3000, 129)])
def test_1nn_through_the_f16_filter(pkg, orc, m, n, k, per_ref):
    q = _u16(100 + k, m, k)
    r = _u16(200 + k, n, k)
    want = _oracle(orc, q, r)
    idx, dist, st = _search(pkg, q, r, path="mfma_perref" if per_ref else "auto")
    assert st["path"] == MFMA and st["k_tile"] == (128 if k <= 128 else 256) and st["filter_form"] == "f16"
    assert st["nonfinite"] == 0
    _same(idx, dist, *want, (m, n, k, per_ref))


@pytest.mark.parametrize("m,n,k", [(5, 1000, 3), (70, 1500, 7), (40, 2000, 128), (64, 600, 300)])
def test_1nn_on_the_exact_path(pkg, orc, m, n, k):
    q = _u16(300 + k, m, k)
    r = _u16(400 + k, n, k)
    idx, dist, st = _search(pkg, q, r)
    assert st["path"] == EXACT and st["filter_form"] == (None if k < 32 or k > 256 else "f16")
    _same(idx, dist, *_oracle(orc, q, r), (m, n, k))
    if k > 256:   # no tile that deep for fp16 points
        with pytest.raises(pkg.NNSError) as e:
            pkg.Index(_dev(r), path="mfma")
        assert e.value.status == UNSUPPORTED


def test_near_ties_go_through_k5s_rerank(pkg, orc):
    k, n, m = 32, 4096, 128
    rng = np.random.default_rng(7)
    vals = np.array([1.0, 1.0 + 2.0 ** -10], np.float16)
    q = vals[rng.integers(0, 2, (m, k))]
    r = vals[rng.integers(0, 2, (n, k))]
    d = v0_all(q.astype(np.float32), r.astype(np.float32))
    tied = ((d == d.min(axis=1, keepdims=True)).sum(axis=1) >= 2).sum()
    assert tied >= 32, tied
    idx, dist, st = _search(pkg, q, r)
    assert st["path"] == MFMA
    assert st["multi_candidate"] + st["ambiguous"] > 0, st
    _same(idx, dist, *_oracle(orc, q, r))


def test_specials(pkg, orc):
    m, n, k = 96, 3000, 64
    q = _u16(1, m, k)
    r0 = _u16(2, n, k)

    def run(qq, rr, path, nonfinite, what):
        idx, dist, st = _search(pkg, qq, rr)
        assert st["path"] == path and st["nonfinite"] == nonfinite, (what, st)
        _same(idx, dist, *_oracle(orc, qq, rr), what)

    r = r0.copy()                                       # NaN and INF among the refs: exact path
    r[5, 3] = np.nan
    r[700, 0] = np.inf
    r[701, 9] = -np.inf
    run(q, r, EXACT, 1, "nan/inf refs")
    r = r0.copy()                                       # values whose -2 v is not finite in binary16
    r[17, 5] = 40000.0
    r[2999, 63] = -65504.0
    run(q, r, EXACT, 1, "refs beyond 32752")
    r = r0.copy()                                       # the largest value the image still holds: the filter runs
    r[17, 5] = 32752.0
    r[18, 6] = -32752.0
    assert float(np.abs(r.astype(np.float32)).max()) == 32752.0
    run(q, r, MFMA, 0, "refs at 32752")
    qs = q.copy()                                       # one INF and one NaN query row among normal ones
    qs[3, 7] = np.inf
    qs[50, 0] = np.nan
    idx, dist, st = _search(pkg, qs, r0)
    assert st["path"] == MFMA and st["nonfinite"] == 1
    want_idx, want_dist = _oracle(orc, qs, r0)
    _same(idx, dist, want_idx, want_dist, "nan/inf queries")
    assert idx[3] == 0 and idx[50] == 0 and np.isinf(dist[3]) and np.isinf(dist[50])   # V0: nothing selectable
    qz, rz = q.copy(), r0.copy()                        # signed zeros
    qz[:, ::3] = np.float16(-0.0)
    rz[:, 1::3] = np.float16(-0.0)
    rz[::2, ::3] = np.float16(0.0)
    run(qz, rz, MFMA, 0, "signed zeros")
    rd, qd = r0.copy(), q.copy()                        # exact duplicates of a query at two indices: the lower wins
    rd[2500] = rd[40]
    qd[9] = rd[40]
    rd[1200] = rd[1999]
    qd[10] = rd[1999]
    idx, dist, st = _search(pkg, qd, rd)
    assert st["path"] == MFMA and idx[9] == 40 and idx[10] == 1200 and dist[9] == 0 and dist[10] == 0
    _same(idx, dist, *_oracle(orc, qd, rd), "duplicates")


def _subnormal_clouds():
    m, n, k = 128, 3000, 64
    rng = np.random.default_rng(31)
    tiny_q = (rng.random((m, k), dtype=np.float32) * np.float32(2.0 ** -14)).astype(np.float16)
    tiny_r = (rng.random((n, k), dtype=np.float32) * np.float32(2.0 ** -14)).astype(np.float16)
    frac = ((tiny_r != 0) & (np.abs(tiny_r.astype(np.float32)) < 2.0 ** -14)).mean()
    assert frac > 0.99, frac
    mix_q, mix_r = _u16(32, m, k), _u16(33, n, k)
    for a, seed in ((mix_q, 34), (mix_r, 35)):
        g = np.random.default_rng(seed)
        mask = g.random(a.shape) < 0.1
        a[mask] = (g.random(int(mask.sum()), dtype=np.float32) * np.float32(2.0 ** -14)).astype(np.float16)
    return {"all_subnormal": (tiny_q, tiny_r), "tenth_subnormal": (mix_q, mix_r)}


@pytest.mark.parametrize("cloud", ["all_subnormal", "tenth_subnormal"])
def test_subnormal_clouds(pkg, orc, cloud):
    q, r = _subnormal_clouds()[cloud]
    want = _oracle(orc, q, r)
    for path in ("auto", "exact"):
        idx, dist, st = _search(pkg, q, r, path=path)
        print(f"{cloud}: path={path} took {st['path']} (nonfinite {st['nonfinite']}, ambiguous {st['ambiguous']})")
        if path == "exact":
            assert st["path"] == EXACT
        _same(idx, dist, *want, (cloud, path))


# ---- top-K and range search ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(3, 70, 3000), (64, 33, 5003)], ids=["k3", "k64"])
def tr_case(request):
    """(q16, r16, V0 distances [m][n], stable order of every row) of one shape, computed once"""
    k, m, n = request.param
    q, r = _u16(500 + k, m, k), _u16(600 + k, n, k)
    r[n // 2] = r[11]                                   # a tie inside every query's list
    d = v0_all(q.astype(np.float32), r.astype(np.float32))
    return q, r, d, np.argsort(d, axis=1, kind="stable")


def test_topk_keys_equal_the_stable_sorted_oracle(pkg, tr_case):
    q, r, d, order = tr_case
    m = q.shape[0]
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
        assert ix.stats()["path"] == EXACT
    with pytest.raises(pkg.NNSError) as e:
        ix.search_topk_keys(qd, 300)
    assert e.value.status == UNSUPPORTED
    idx, dist = ix.search_topk(qd, 10, return_distances=True)
    torch.cuda.synchronize()
    assert np.array_equal(idx.cpu().numpy(), order[:, :10]) and idx.shape == (m, 10)
    assert np.array_equal(_bits(dist.cpu().numpy()), _bits(np.take_along_axis(d, order[:, :10], 1)))
    ix.close()


def test_range_search_matches_the_range_oracle(pkg, tr_case):
    q, r, d, order = tr_case
    m, n = d.shape
    radius2 = float(np.sort(d, axis=None)[20 * m])      # about 20 hits per query
    want = range_oracle(q.astype(np.float32), r.astype(np.float32), radius2)
    assert 10 * m <= want[0][-1] <= 40 * m
    ix = pkg.Index(_dev(r))
    qd = _dev(q)
    lims, idx, dist = ix.search_range(qd, radius2, return_distances=True)
    torch.cuda.synchronize()
    assert np.array_equal(lims.cpu().numpy(), want[0])
    assert np.array_equal(idx.cpu().numpy(), want[1])
    assert np.array_equal(_bits(dist.cpu().numpy()), _bits(want[2]))
    # a fill after a count with zero hits succeeds (null output pointers are not written)
    far = _dev((q.astype(np.float32) + 100.0).astype(np.float16))
    lims0 = ix.range_count(far, 0.5)
    torch.cuda.synchronize()
    assert int(lims0[-1].item()) == 0 and not lims0.cpu().numpy().any()
    out = ix.range_fill(far, 0.5, lims0, total=0, return_distances=True)
    torch.cuda.synchronize()
    assert out[0].numel() == 0 and out[1].numel() == 0
    ix.close()


# ---- whole calls ----------------------------------------------------------------------------------------------------
def test_whole_calls(pkg, orc):
    m, n, k = 130, 5003, 100
    q, r = _u16(71, m, k), _u16(72, n, k)
    want = _oracle(orc, q, r)
    for shards in (1, 3):
        idx, dist = pkg.search_f16(q, r, return_distances=True, shards=shards)
        _same(idx, dist, *want, shards)
    assert np.array_equal(pkg.search_f16(q.view(np.uint16), r.view(np.uint16)), want[0])       # raw bit patterns
    idx, dist = pkg.search_f16(q, np.ascontiguousarray(r.T), return_distances=True, refs_soa=True)
    _same(idx, dist, *want, "soa")
    idx, dist = pkg.search_f16(q, r, return_distances=True, path="exact")
    _same(idx, dist, *want, "exact")
    d = v0_all(q.astype(np.float32), r.astype(np.float32))
    order = np.argsort(d, axis=1, kind="stable")[:, :7]
    assert np.array_equal(pkg.search_topk_f16(q, r, 7), order)
    idx, dist = pkg.search_topk_f16(q, r, 7, return_distances=True, shards=2)
    assert np.array_equal(idx, order) and np.array_equal(_bits(dist), _bits(np.take_along_axis(d, order, 1)))
    radius2 = float(np.sort(d, axis=None)[20 * m])
    wl, wi, wd = range_oracle(q.astype(np.float32), r.astype(np.float32), radius2)
    lims, idx = pkg.search_range_f16(q, r, radius2)
    assert np.array_equal(lims, wl) and np.array_equal(idx, wi)
    lims, idx, dist = pkg.search_range_f16(q, r, radius2, return_distances=True)
    assert np.array_equal(lims, wl) and np.array_equal(idx, wi) and np.array_equal(_bits(dist), _bits(wd))
    with pytest.raises(ValueError):
        pkg.search_f16(q.astype(np.float32), r)


# ---- the resident index's lifecycle ---------------------------------------------------------------------------------
def _keys_of(d, sel, base=0):
    """packed keys of the entries sel [m][kn] of the distance matrix d"""
    dv = np.take_along_axis(d, sel, 1)
    return (dv.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (sel + base).astype(np.uint64)


def lifecycle_common(pkg, orc, q, r, q_many, r_new, form, plan_dtype):
    """What test_b1_gpu.test_split_api_manners checks, for an index that runs an MFMA filter (also the body of
    test_i8_gpu's lifecycle test).  q, r, q_many, r_new: points in the index's own numpy dtype, (130, 5003, 100) with 700
    queries in q_many; form: stats()["filter_form"]; plan_dtype: plan_filter's bf16 argument.  One index with
    index_base 10^6 serves 1-NN, top-5, a range search and search_indices on a caller's stream, then m = 40 (below 64
    queries: the exact kernels), 700 (m_pad beyond 512: the query workspace and the lists grow) and 130 again; two half
    indices merge to a whole one's keys; a refresh() follows refs rewritten in place.  Every answer is the V0 oracle's,
    bit for bit.  Returns (ix, rd, qd, base), the index still open on r_new."""
    f = lambda a: a.astype(np.float32)                  # noqa: E731
    m, n, k = q.shape[0], r.shape[0], r.shape[1]
    want = orc.v0_search(f(q), f(r))
    d = v0_all(f(q), f(r))
    base = 10 ** 6
    rd, qd = _dev(r), _dev(q)
    before = torch.cuda.current_device()
    ix = pkg.Index(rd, index_base=base, profile=True)
    torch.cuda.synchronize()
    radius2 = float(np.sort(d, axis=None)[10 * m])      # about 10 hits per query
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        keys = ix.search_keys(qd, stream=st)
        tk = ix.search_topk_keys(qd, 5, stream=st)
        lims, ridx, rdist = ix.search_range(qd, radius2, return_distances=True, stream=st)
        idx = ix.search_indices(qd, stream=st)
    st.synchronize()
    assert np.array_equal(keys.cpu().numpy().view(np.uint64), _keys_of(d, want[0][:, None].astype(np.int64), base)[:, 0])
    oi, _ = topk_oracle(f(q), f(r), 5)
    assert np.array_equal(tk.cpu().numpy().view(np.uint64), _keys_of(d, oi.astype(np.int64), base))
    wl, wi, wd = range_oracle(f(q), f(r), radius2, index_base=base)
    assert 5 * m <= wl[-1] <= 20 * m
    assert np.array_equal(lims.cpu().numpy(), wl) and np.array_equal(ridx.cpu().numpy(), wi)
    assert np.array_equal(_bits(rdist.cpu().numpy()), _bits(wd))
    assert np.array_equal(idx.cpu().numpy(), want[0] + base)
    s = ix.stats()
    assert s["path"] == MFMA and s["filter_form"] == form and s["nonfinite"] == 0, s
    assert torch.cuda.current_device() == before

    def check(qq, path, what):
        i, dd = ix.search(_dev(qq), return_distances=True)
        torch.cuda.synchronize()
        _same(i.cpu().numpy() - base, dd.cpu().numpy(), *orc.v0_search(f(qq), f(r)), what)
        s = ix.stats()
        assert s["path"] == path and s["nonfinite"] == 0, (what, s)

    # one index, changing m
    pads = [pkg.plan_filter(k, mm, n, bf16=plan_dtype)["m_pad"] for mm in (m, q_many.shape[0])]
    assert pads[0] <= 512 < pads[1], pads
    check(q[:40], EXACT, "m = 40")
    check(q_many, MFMA, "m = 700")
    check(q, MFMA, "m = 130 again")
    # shards: two half indices over an odd n, merged, against a whole index with base 0
    whole = pkg.Index(rd)
    wk, wtk = whole.search_keys(qd), whole.search_topk_keys(qd, 5)
    torch.cuda.synchronize()
    whole.close()
    assert np.array_equal(wk.cpu().numpy().view(np.uint64), _keys_of(d, want[0][:, None].astype(np.int64))[:, 0])
    assert np.array_equal(wtk.cpu().numpy().view(np.uint64), _keys_of(d, oi.astype(np.int64)))
    h = n // 2
    assert n % 2 == 1
    lo, hi = pkg.Index(rd[:h]), pkg.Index(rd[h:], index_base=h)
    a, b = lo.search_keys(qd), hi.search_keys(qd)
    pkg.keys_min(a, b)
    torch.cuda.synchronize()
    assert lo.stats()["path"] == MFMA and hi.stats()["path"] == MFMA      # (of the 1-NN searches: both halves filtered)
    ta, tb = lo.search_topk_keys(qd, 5), hi.search_topk_keys(qd, 5)
    pkg.keys_topk_merge(ta, tb)
    torch.cuda.synchronize()
    lo.close()
    hi.close()
    assert torch.equal(a, wk) and torch.equal(ta, wtk)
    # refresh() after rewriting the refs in place
    rd.copy_(torch.from_numpy(r_new))
    ix.refresh()
    i2, d2 = ix.search(qd, return_distances=True)
    torch.cuda.synchronize()
    _same(i2.cpu().numpy() - base, d2.cpu().numpy(), *orc.v0_search(f(q), f(r_new)), "after refresh")
    s = ix.stats()
    assert s["path"] == MFMA and s["filter_form"] == form and s["nonfinite"] == 0, s
    return ix, rd, qd, base


def test_resident_index_lifecycle(pkg, orc):
    """lifecycle_common for fp16 points, then the stale-flag window of a refresh (test_refresh_relatches_nonfinite_refs
    for fp16): refs rewritten to hold one 40000.0 — finite, but -2 v is not in binary16 — are caught on the device by K5
    while the host still believes the image clean; stats() re-latches, and a clean refresh brings the filter back."""
    m, n, k = 130, 5003, 100
    q, r, r_new = _u16(91, m, k), _u16(92, n, k), _u16(94, n, k)
    ix, rd, qd, base = lifecycle_common(pkg, orc, q, r, _u16(93, 700, k), r_new, "f16", 2)
    r_big = r_new.copy()
    r_big[1234, 7] = 40000.0
    assert np.isfinite(r_big.astype(np.float32)).all() and float(r_big[1234, 7]) == 40000.0
    want_big = _oracle(orc, q, r_big)
    rd.copy_(torch.from_numpy(r_big))
    ix.refresh()                                        # no stats() from here to the search: the host flag is stale
    i, d = ix.search(qd, return_distances=True)
    torch.cuda.synchronize()
    _same(i.cpu().numpy() - base, d.cpu().numpy(), *want_big, "stale flag")
    s = ix.stats()
    assert s["nonfinite"] == 1 and s["ambiguous"] == m, s           # the device-side check sent every query to the scan
    i, d = ix.search(qd, return_distances=True)
    torch.cuda.synchronize()
    _same(i.cpu().numpy() - base, d.cpu().numpy(), *want_big, "re-latched")
    assert ix.stats()["path"] == EXACT                  # re-latched by stats(): straight to the exact kernels now
    rd.copy_(torch.from_numpy(r))
    ix.refresh()
    i, d = ix.search(qd, return_distances=True)
    torch.cuda.synchronize()
    _same(i.cpu().numpy() - base, d.cpu().numpy(), *_oracle(orc, q, r), "clean again")
    s = ix.stats()
    assert s["path"] == MFMA and s["nonfinite"] == 0 and s["filter_form"] == "f16", s
    ix.close()


def test_dtype_mismatch(pkg):
    m, n, k = 64, 512, 64
    q, r = _u16(81, m, k), _u16(82, n, k)
    ix = pkg.Index(_dev(r))
    keys = torch.empty(m, dtype=torch.int64, device=DEV)
    for wrong in (torch.bfloat16, torch.float32):
        qw = _dev(q).to(wrong)
        with pytest.raises(ValueError):
            ix.search(qw)
        with pytest.raises(ValueError):
            ix.search_topk(qw, 3)
        with pytest.raises(ValueError):
            ix.range_count(qw, 1.0)
    qd = _dev(q)
    L = pkg.lib
    assert L.nns_index_search(ix._h, m, qd.data_ptr(), keys.data_ptr(), None) == INVALID
    assert L.nns_index_search_bf16(ix._h, m, qd.data_ptr(), keys.data_ptr(), None) == INVALID
    assert L.nns_index_search_f16(ix._h, m, qd.data_ptr(), keys.data_ptr(), None) == 0
    torch.cuda.synchronize()
    ix.close()
    for other in (torch.bfloat16, torch.float32):       # and the reverse
        ixo = pkg.Index(_dev(r).to(other))
        with pytest.raises(ValueError):
            ixo.search(qd)
        assert L.nns_index_search_f16(ixo._h, m, qd.data_ptr(), keys.data_ptr(), None) == INVALID
        ixo.close()
