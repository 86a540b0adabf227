"""GPU tests of the int8 pre-pass of the lazy split filter (filter_i8pre_kernel, OpI8Pre: KT = 128, long-stream record form).
Small shapes reach it through path="mfma_perref", as tests/test_lazy16_gpu.py's do; every test asserts what
Index.filter_pre() must say.  Indices and distance bits are V0's (the oracle); keys equal those of the other schedules."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_filter_configs_gpu import _bits, v0_rows  # noqa: E402
from test_lazy16_gpu import SHAPES, _check_vs_v0, _require_lazy16, _ulp_up, _uniform  # noqa: E402
from test_split_filter_cpu import _split  # noqa: E402

pytestmark = pytest.mark.gpu


def _search(pkg, q, r, want_pre, **kw):
    """(keys, idx, dist) of one search on the forced MFMA path with per-score records; filter_pre() must say want_pre."""
    ix = pkg.Index(torch.from_numpy(r).cuda(), path="mfma_perref", **kw)
    keys = ix.search_keys(torch.from_numpy(q).cuda()).clone()
    torch.cuda.synchronize()
    st = ix.stats()
    assert ix.filter_pre() == want_pre, (kw, st)
    ix.close()
    assert st["path"] == 2 and st["k_tile"] == 128 and st["nonfinite"] == 0, st
    idx, dist = pkg.keys_unpack(keys, return_distances=True)
    return keys, idx.cpu().numpy(), dist.cpu().numpy(), st


_cache = {}


def _shape_run(pkg, name):
    """(q, r, keys, idx, dist) of the forced pre-pass search of a shape: computed once, shared, not modified."""
    if name not in _cache:
        m, n, k = SHAPES[name]
        _require_lazy16(pkg, m, n, k)
        q, r = _uniform(pkg, m, n, k, 2600 + len(name))
        keys, idx, dist, _ = _search(pkg, q, r, True, filter_i8pre="force")
        _cache[name] = (q, r, keys, idx, dist)
    return _cache[name]


@pytest.mark.parametrize("name", list(SHAPES))
def test_i8pre_shapes_vs_v0(pkg, orc, name):
    """One-slot streams; padded queries, refs and dims; several turns of the ring of sixteen with retiring tiles in the
    previous slot (the oracle on 512 spread queries there)."""
    q, r, _, idx, dist = _shape_run(pkg, name)
    m = q.shape[0]
    sel = None if m <= 1024 else np.arange(5, m, m // 512)
    _check_vs_v0(orc, q, r, idx, dist, sel)


@pytest.mark.parametrize("name", list(SHAPES))
def test_i8pre_keys_equal_the_other_schedules(pkg, name):
    q, r, keys, _, _ = _shape_run(pkg, name)
    auto, _, _, _ = _search(pkg, q, r, True)                       # uniform clouds pass the selection rule
    assert torch.equal(keys, auto)
    for kw in ({"filter_i8pre": "off"}, {"filter_split_eager": True}, {"filter_f32": True}):
        other, _, _, _ = _search(pkg, q, r, False, **kw)
        assert torch.equal(keys, other), kw


def test_i8pre_outlier_coordinate_declines_under_auto_and_is_exact_under_force(pkg, orc):
    """One ref coordinate 1000 x the rest: the shared scale leaves the other 127 dimensions no resolution, every query's
    bound is far above 1.5 B and "auto" runs lazy16; "force" runs the pre-pass and still returns V0's answers."""
    m, n, k = 512, 4096, 128
    _require_lazy16(pkg, m, n, k)
    q, r = _uniform(pkg, m, n, k, 2701)
    r = r.copy()
    r[:, 7] *= np.float32(1000.0)
    for mode, want in (("auto", False), ("force", True)):
        _, idx, dist, _ = _search(pkg, q, r, want, filter_i8pre=mode)
        _check_vs_v0(orc, q, r, idx, dist)


def test_i8pre_clipped_queries(pkg, orc):
    """Queries scaled x 3 lie outside the refs' range in most coordinates: q8 clips, the clipped part is in e_x and so in
    B8.  All of them clipped: V0's answers under "force".  m / 64 of them clipped: the count stays within the rule and
    "auto" keeps the pre-pass."""
    m, n, k = 512, 4096, 128
    _require_lazy16(pkg, m, n, k)
    q, r = _uniform(pkg, m, n, k, 2702)
    q3 = (q * np.float32(3.0)).astype(np.float32)
    _, idx, dist, _ = _search(pkg, q3, r, True, filter_i8pre="force")
    _check_vs_v0(orc, q3, r, idx, dist)
    qs = q.copy()
    qs[:: 64][: m // 64] = q3[:: 64][: m // 64]
    _, idx, dist, _ = _search(pkg, qs, r, True)
    _check_vs_v0(orc, qs, r, idx, dist)


def test_i8pre_lifecycle_refresh_and_changing_m(pkg, orc):
    """refresh() after the refs were rescaled x 4 and then x 1/16 (scale, seeds and the uint-ordered maxima must follow in
    both directions: stale larger words would inflate every bound and "auto" would decline), fewer and more queries on one
    index, and index_base on a caller stream."""
    m, n, k = 512, 4096, 128
    _require_lazy16(pkg, m, n, k)
    q, r = _uniform(pkg, m, n, k, 2703)
    rt = torch.from_numpy(r).cuda()
    base = 1000
    ix = pkg.Index(rt, path="mfma_perref", index_base=base)
    cs = torch.cuda.Stream()

    def check(qn, rn):
        qd = torch.from_numpy(qn).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(cs):
            keys = ix.search_keys(qd, stream=cs).clone()
        cs.synchronize()
        assert ix.filter_pre()
        idx, dist = pkg.keys_unpack(keys, return_distances=True)
        idx = idx.cpu().numpy().astype(np.int64)
        assert idx.min() >= base
        _check_vs_v0(orc, qn, rn, idx - base, dist.cpu().numpy())

    check(q, r)
    rt.mul_(4.0)
    torch.cuda.synchronize()
    ix.refresh()
    r4 = (r * np.float32(4.0)).astype(np.float32)
    q4 = (q * np.float32(4.0)).astype(np.float32)
    check(q4, r4)
    check(q4[:200], r4)
    q2, _ = _uniform(pkg, 1024, 64, k, 2704)
    check((q2 * np.float32(4.0)).astype(np.float32), r4)
    rt.mul_(1.0 / 16.0)
    torch.cuda.synchronize()
    ix.refresh()
    check((q * np.float32(0.25)).astype(np.float32), (r * np.float32(0.25)).astype(np.float32))
    ix.close()


def test_i8pre_nan_ref_and_nan_query_behave_as_lazy16(pkg):
    """A NaN among the refs voids the scale (lazy16 runs; K5 sends the queries to the exact scan as before); a NaN in one
    query leaves the other queries' keys what "off" gives."""
    m, n, k = 512, 4096, 128
    _require_lazy16(pkg, m, n, k)
    q, r = _uniform(pkg, m, n, k, 2705)
    rn = r.copy()
    rn[1234, 5] = np.nan
    qn = q.copy()
    qn[77, 3] = np.nan
    for qq, rr in ((q, rn), (qn, r)):
        got = {}
        for mode in ("auto", "off"):
            ix = pkg.Index(torch.from_numpy(rr).cuda(), path="mfma_perref", filter_i8pre=mode)
            got[mode] = ix.search_keys(torch.from_numpy(qq).cuda()).clone()
            torch.cuda.synchronize()
            # (NaN refs: no filter at all; a NaN query leaves the scale valid and counts as one odd query: the pre-pass runs)
            assert ix.filter_pre() == (rr is r and mode == "auto")
            ix.close()
        assert torch.equal(got["auto"], got["off"])


# ---- the chain on hardware ------------------------------------------------------------------------------------------
def test_i8pre_chain_on_one_wave_equals_int64(pkg):
    """selftest_mfma_i8pre: 32 refs x 64 queries at kt = 128 through K2's lane map (refs negated) and the operator's own seed
    and accumulate MFMAs; asymmetric full-range operands (-128 is not produced by K2 but the MFMA must take -127 .. 127
    of either sign in any byte position) and nonzero seeds of both signs.  Accumulators equal numpy's int64."""
    rng = np.random.default_rng(2800)
    q = rng.integers(-127, 128, (64, 128)).astype(np.int8)
    r = rng.integers(-127, 128, (32, 128)).astype(np.int8)
    q[:, ::3] = np.abs(q[:, ::3])                        # asymmetric: no sign pattern cancels a lane-map mistake
    r[5], r[21], q[9], q[40] = 127, -127, 127, -127      # the extreme dot products, +-128 * 127^2
    seeds = rng.integers(-(1 << 20), 1 << 20, 32).astype(np.int32)
    seeds[0], seeds[31] = 0x3FFFFFFF - 128 * 127 * 127, -(1 << 29)
    out = pkg.selftest_mfma_i8pre(q, r, seeds)
    want = seeds.astype(np.int64)[:, None] - r.astype(np.int64) @ q.astype(np.int64).T
    assert np.array_equal(out.astype(np.int64), want), np.argwhere(out != want)[:5]


# ---- every owner and partner quarter, both ref tiles, all four states ---------------------------------------------------
def test_i8pre_planted_neighbours_cover_every_quarter_and_state(pkg, orc):
    """test_lazy16_planted_neighbours_cover_every_quarter_and_state's construction under the pre-pass: query i has a
    near-duplicate ref at block i % 128, row (4 (i // 64) + i % 64) % 32 — every query residue mod 64 (four states x 16
    columns) meets all eight row quarters (both ref tiles x g = 0 .. 3: owners' rows and rows handed over by a partner)."""
    m, n, k = 512, 4096, 128
    _require_lazy16(pkg, m, n, k)
    q, r = _uniform(pkg, m, n, k, 2810)
    i = np.arange(m)
    rows = (4 * (i // 64) + i % 64) % 32
    j = 32 * (i % 128) + rows
    assert np.unique(j).size == m and set(rows) == set(range(32))
    assert {(c, qr) for c, qr in zip(i % 64, rows // 4)} == {(c, qr) for c in range(64) for qr in range(8)}
    r[j] = q
    for t in range(m):
        r[j[t], t % k] = _ulp_up(r[j[t], t % k])
    _, idx, dist, _ = _search(pkg, q, r, True, filter_i8pre="force")
    assert np.array_equal(idx, j), np.nonzero(idx != j)[0][:8]
    _check_vs_v0(orc, q, r, idx, dist)


def test_i8pre_ties_over_the_four_lane_quarters(pkg, orc):
    """Eight exact copies of a query's nearest ref in one 32-ref block, two in each lane quarter: the answer is V0's — the
    lowest index."""
    m, n, k = 512, 4096, 128
    _require_lazy16(pkg, m, n, k)
    q, r = _uniform(pkg, m, n, k, 2820)
    copies = np.array([1, 6, 9, 14, 17, 22, 27, 30])
    assert sorted((copies % 16) // 4) == [0, 0, 1, 1, 2, 2, 3, 3]
    group = np.array([3, 64 + 19, 128 + 37, 192 + 60, 448 + 8, 500])       # all four states, several waves
    blocks = np.array([0, 17, 63, 64, 100, 127])
    for g, b in zip(group, blocks):
        r[32 * b + copies] = q[g]
    _, idx, dist, _ = _search(pkg, q, r, True, filter_i8pre="force")
    assert np.array_equal(idx[group], 32 * blocks + 1), idx[group]
    assert (dist[group] == 0).all()
    _check_vs_v0(orc, q, r, idx, dist)


def test_i8pre_monotone_stream_wraps_the_lists(pkg, orc):
    """test_lazy16_monotone_stream_wraps_the_lists under "force": 64 identical queries and refs at strictly decreasing
    distance — every tile refines, the lists wrap; in the second half every ref is within the margin of the last one, the
    overflow bit sends every query to the exact scan.  Keys are V0's: the last ref."""
    m, n, k = 64, 65536, 128
    p = _require_lazy16(pkg, m, n, k)
    assert p["slots_per_split"] * p["slot_pts"] == 256, p
    rng = np.random.default_rng(19)
    x = (rng.random(k, dtype=np.float32) * np.float32(0.5) + np.float32(0.25)).astype(np.float32)
    q = np.repeat(x[None, :], m, axis=0)
    r = np.repeat(x[None, :], n, axis=0)
    h = n // 2
    r[:h] += np.linspace(1.0, 0.5, h, dtype=np.float32)[:, None]
    r[np.arange(h, n), np.arange(h, n) % k] += np.linspace(2e-2, 1e-2, n - h, dtype=np.float32)
    d = v0_rows(np.repeat(x[None, :], n, axis=0), r)
    assert (np.diff(d) < 0).all(), "V0's distances are not strictly decreasing"
    c = r.astype(np.float64).mean(0)
    c0, _, _ = pkg.tau_consts(k, float(((x - c) ** 2).sum()), float(((r - c) ** 2).sum(1).max()), 3)
    assert d[h] - d[-1] < 0.25 * c0, (d[h], d[-1], c0)
    _, idx, dist, st = _search(pkg, q, r, True, filter_i8pre="force")
    assert (idx == n - 1).all(), idx
    assert st["ambiguous"] == m, st
    _check_vs_v0(orc, q, r, idx, dist)


@pytest.mark.parametrize("t_row", [5, 21])
def test_i8pre_true_nearest_ref_needs_the_bound(pkg, orc, t_row):
    """(512, 8192, 128), one-slot streams.  The refs are a set and its mirror image (mean 0, largest |coordinate| 1: the
    scale is s = (1 + 2^-22) / 127).  One query group and its true nearest ref T sit, in every coordinate, just below the
    rint midpoint 100.5 s (q8 = r8 = 100, e = +1/2 throughout: all three cross terms of the bound aligned), so T's
    integer accumulator overstates its score by nearly B8 (0.97 B8 on this family: tests/test_i8pre_cpu.py).  E, in the block
    before T in the same stream, is farther by 0.06 — more than twice the summation slack of 0.02, so that T is the nearer
    one to the three-product filter too.  In numpy first: 2 s^2 A_T lies above the threshold E leaves by more than 0.85 B8
    (0.97 B8 less the 0.06, the margin tau ~ 0.04 and the slack, together 0.08 B8), and B8 covers it.  T sits in a row quarter whose lane owns no list."""
    m, n, k = 512, 8192, 128
    p = _require_lazy16(pkg, m, n, k)
    assert p["slots_per_split"] == 1 and p["slot_pts"] == 64, p
    F, U = np.float32, 2.0 ** -24
    rng = np.random.default_rng(2830)
    half = (rng.integers(-2 ** 15, 2 ** 15, (n // 2, k)) * 2.0 ** -16).astype(F)
    s0 = F(1.0) / F(127.0)
    qg = np.full(k, F(100.5) * s0, F)
    T = qg.copy()
    E = (qg + F(0.0217) * np.where(np.arange(k) % 2 == 0, 1, -1)).astype(F)   # farther by 128 * 0.0217^2 = 0.06
    jE, jT = 64 * 10 + 2, 64 * 10 + 32 + t_row
    half[jE], half[jT] = E, T
    half[0, 0] = F(1.0)                                   # fixes cmax
    r = np.concatenate([half, -half]).astype(F)
    q = rng.random((m, k), dtype=F) - F(0.5)
    grp = np.arange(128, 128 + 64)
    q[grp] = qg
    d = lambda t: t.astype(np.float64)   # noqa: E731
    # K2's quantisation, in its fp32 arithmetic (the mean of a set and its mirror image is 0 up to ~1e-17)
    cmax = F(F(1.0) * F(1.0 + 2.0 ** -22))
    s, inv = F(cmax / F(127.0)), F(F(127.0) / cmax)
    quant = lambda v: np.clip(np.rint((v * inv).astype(F)), -127, 127)   # noqa: E731
    t8 = (T * inv).astype(F)
    assert (quant(T) == 100).all() and ((t8 - 100 > 0.4999) & (t8 - 100 < 0.5)).all()
    r8, q8 = quant(r).astype(np.int64), quant(qg).astype(np.int64)
    ey2 = ((d((r * inv).astype(F)) - r8) ** 2).sum(1)
    ex2 = float(((d((qg * inv).astype(F)) - q8) ** 2).sum())
    X2, ymax2 = float((d(qg) ** 2).sum()), float((d(r) ** 2).sum(1).max())
    c0, c1, x2 = pkg.tau_consts(k, X2, ymax2, 3)
    B8 = pkg.i8pre_bound(float(s), ex2 * (1 + 2.0 ** -20), float((q8 ** 2).sum()), float((r8 ** 2).sum(1).max()),
                         float(ey2.max() * (1 + 2.0 ** -20)), c0)
    unit = 2.0 * float(s) ** 2
    A_T = np.floor((d(T) ** 2).sum() / unit) - float(q8 @ quant(T).astype(np.int64))
    qh, ql = _split(qg)

    def s3(y):
        vh, vl = _split((F(-2) * y).astype(F))
        return float((d(y) ** 2).sum() + d(qh) @ d(vh) + d(qh) @ d(vl) + d(ql) @ d(vh))
    s3_E, s3_T = s3(E), s3(T)
    acc_slack = 2 * (3 * k + 3 * (k // 16) + 2) * U * (ymax2 + 4 * np.sqrt(X2 * ymax2))   # hardware summation
    thr_E = s3_E + acc_slack + 1.002 * (c0 + c1 * max(s3_E + acc_slack + x2, 0.0)) * (1 + 4 * U)
    assert s3_T + acc_slack < s3_E - acc_slack                 # T is the nearer one also to the filter
    assert A_T * unit - thr_E > 0.85 * B8, (A_T * unit, thr_E, B8)   # ... its integer score is far above the threshold E leaves
    assert A_T * unit - (s3_T + acc_slack) <= B8               # and B8 is what brings its tile back
    want_idx, want_dist = orc.v0_search(q[grp], r, threads=16)
    assert (want_idx == jT).all() and (want_dist == 0).all()
    _, idx, dist, _ = _search(pkg, q, r, True, filter_i8pre="force")
    assert np.array_equal(idx[grp], want_idx), idx[grp]
    assert np.array_equal(_bits(dist[grp]), _bits(want_dist))
