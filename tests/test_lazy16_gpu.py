"""GPU tests of the lazy split filter on 16x16x32 MFMAs (filter_lazy16_kernel, OpLazySplit16: the default lazy kernel at
KT = 128).  Small shapes reach it through path="mfma_perref" (per-score records, the lazy schedule's condition); every
test first requires the plan to say lazy and the build to say tile 16.  Indices and distance bits are V0's (the oracle).
What is particular to this kernel: a query sits on FOUR lanes (row quarters g = 0 .. 3 of each 16-ref tile) but keeps TWO
lists, owned by the even quarters, to which the odd quarters hand their refined scores; operands are gathered out of an
image in the 32x32x16 order; the retiring tile may sit in the previous ring slot."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_filter_configs_gpu import _bits, v0_rows  # noqa: E402
from test_split_filter_cpu import _families, _split  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
KT = 128


def _require_lazy16(pkg, m, n, k):
    p = pkg.plan_filter(k, m, n, flags=pkg.NNS_RECORDS_PER_REF, schedule=True)
    assert p["lazy"] == 1 and p["kt"] == KT and p["tile_rec"] == 0 and p["lpq"] == 2, p
    assert pkg.filter_lazy_tile() == 16
    return p


def _uniform(pkg, m, n, k, seed):
    q = torch.empty((m, k), dtype=torch.float32, device="cuda")
    r = torch.empty((n, k), dtype=torch.float32, device="cuda")
    pkg.fill_uniform(q, seed, 0)
    pkg.fill_uniform(r, seed, m * k)
    out = q.cpu().numpy(), r.cpu().numpy()
    del q, r
    return out


def _search(pkg, q, r, **kw):
    """(keys, idx, dist, stats) of one search on the forced MFMA path with per-score records."""
    ix = pkg.Index(torch.from_numpy(r).cuda(), path="mfma_perref", **kw)
    keys = ix.search_keys(torch.from_numpy(q).cuda()).clone()
    torch.cuda.synchronize()
    st = ix.stats()
    ix.close()
    assert st["path"] == 2 and st["k_tile"] == KT and st["nonfinite"] == 0, st
    idx, dist = pkg.keys_unpack(keys, return_distances=True)
    return keys, idx.cpu().numpy(), dist.cpu().numpy(), st


def _check_vs_v0(orc, q, r, idx, dist, sel=None):
    """Every query's distance is V0's arithmetic on its answer; the queries `sel` (default: all) agree with the oracle."""
    assert idx.min() >= 0 and idx.max() < r.shape[0]
    assert np.array_equal(_bits(v0_rows(q, r[idx])), _bits(dist))
    sel = np.arange(q.shape[0]) if sel is None else np.asarray(sel)
    want_idx, want_dist = orc.v0_search(q[sel], r, threads=16)
    assert np.array_equal(idx[sel], want_idx), sel[np.nonzero(idx[sel] != want_idx)[0][:5]]
    assert np.array_equal(_bits(dist[sel]), _bits(want_dist))


# ---- the chain on hardware ------------------------------------------------------------------------------------------
def test_lazy16_chain_error_model_and_bound(pkg):
    """selftest_mfma_lazy16 (operands gathered out of images in the 32x32x16 order, four hi.hi MFMAs of 32 dims, then
    rh.ql and rl.qh per step on the same accumulator) on the input families of
    test_lazy_mfma_chain_error_model_and_bound at kt = 128: accumulation error within 1/4 of the 2u-per-add bound of the
    mode-3 model, total error within mode 3's e3 + e2, and s_hh - s_3 <= B for every (ref, query) pair."""
    assert pkg.filter_lazy_tile() == 16
    kt = KT
    rng = np.random.default_rng(57 + kt)
    na = 3 * kt + 3 * (kt // 16) + 2
    worst_acc = worst_b = 0.0
    for name, x1, v1 in _families(rng, kt):
        if name.startswith("subnormal"):
            continue   # (denormal handling of the MFMA: the floor of tau and B; tests/test_underflow_gpu.py)
        x = np.stack([x1[rng.permutation(kt)] for _ in range(64)]).astype(np.float32)                    # queries
        v = np.stack([v1[rng.permutation(kt)] * np.float32(1 if i % 3 else -1) for i in range(32)]).astype(np.float32)
        c0 = ((v.astype(np.float64) / 2) ** 2).sum(1).astype(np.float32)   # |y'|^2, v = -2 y'
        out, out_hh = pkg.selftest_mfma_lazy16(x, v, c0)                   # [ref i][query j]
        out, out_hh = out.astype(np.float64), out_hh.astype(np.float64)
        vh, vl = _split(v)
        xh, xl = _split(x)
        d = lambda t: t.astype(np.float64)   # noqa: E731
        prods = d(vh) @ d(xh).T + d(vh) @ d(xl).T + d(vl) @ d(xh).T
        absprods = np.abs(d(vh)) @ np.abs(d(xh)).T + np.abs(d(vh)) @ np.abs(d(xl)).T + np.abs(d(vl)) @ np.abs(d(xh)).T
        acc_err = np.abs(out - (d(c0)[:, None] + prods))
        acc_bound = 2 * na * U * (np.abs(d(c0))[:, None] + absprods)
        print(f"lazy16 chain {name}: accumulation error / bound {float((acc_err / acc_bound).max()):.4f}")
        assert (acc_err <= 0.25 * acc_bound).all(), (name, float((acc_err / acc_bound).max()))
        worst_acc = max(worst_acc, float((acc_err / acc_bound).max()))
        hh_err = np.abs(out_hh - (d(c0)[:, None] + d(vh) @ d(xh).T))
        assert (hh_err <= 0.25 * acc_bound).all(), name
        tot_err = np.abs(out - (d(c0)[:, None] + d(v) @ d(x).T))
        y2max = float(c0.max())
        for j in range(64):
            x2 = float((d(x[j]) ** 2).sum())
            c0t, c1t, _ = pkg.tau_consts(kt, x2, y2max, 3)
            assert tot_err[:, j].max() <= c0t / (2.0 + c1t) / 1.001, (name, j)
            B = pkg.split_lazy_bound(kt, x2, y2max)
            gap = float((out_hh[:, j] - out[:, j]).max())
            assert gap <= B, (name, j, gap, B)
            worst_b = max(worst_b, gap / B)
    print(f"lazy16 chain: accumulation error / 2u-per-add bound {worst_acc:.4f}, (s_hh - s_3) / B {worst_b:.4f}")


# ---- shapes against V0, and the other operand forms ---------------------------------------------------------------------
SHAPES = {
    "one_slot_streams": (200, 5000, 128),     # streams of one slot: the first interval and the tail only
    "padded": (513, 4097, 100),               # padded queries, padded refs (+INF norms), zero-padded dims
    "ring_turns": (8192, 65536, 128),         # 64 slots per stream: several turns of the ring of eight
}
_cache = {}


def _shape_run(pkg, name):
    """(q, r, keys, idx, dist) of the default (lazy, tile 16) search of a shape: computed once, shared, not modified."""
    if name not in _cache:
        m, n, k = SHAPES[name]
        _require_lazy16(pkg, m, n, k)
        q, r = _uniform(pkg, m, n, k, 1600 + len(name))
        keys, idx, dist, st = _search(pkg, q, r)
        assert st["filter_form"] == "split", st
        _cache[name] = (q, r, keys, idx, dist)
    return _cache[name]


@pytest.mark.parametrize("name", list(SHAPES))
def test_lazy16_shapes_vs_v0(pkg, orc, name):
    q, r, _, idx, dist = _shape_run(pkg, name)
    m = q.shape[0]
    # (the oracle over all queries of the small shapes; 512 of the large one's, spread over every workgroup)
    sel = None if m <= 1024 else np.arange(5, m, m // 512)
    _check_vs_v0(orc, q, r, idx, dist, sel)


@pytest.mark.parametrize("name", ["one_slot_streams", "padded"])
def test_lazy16_keys_equal_the_eager_split_and_the_fp32_operand_forms(pkg, name):
    q, r, keys, _, _ = _shape_run(pkg, name)
    for kw, form in (({"filter_split_eager": True}, "split"), ({"filter_f32": True}, "fp32")):
        other, _, _, st = _search(pkg, q, r, **kw)
        assert st["filter_form"] == form, st
        assert torch.equal(keys, other), kw


# ---- every owner and partner quarter, both ref tiles, all four states ---------------------------------------------------
def _ulp_up(v, u=1):
    return (np.array([v], np.float32).view(np.uint32) + np.uint32(u)).view(np.float32)[0]


def test_lazy16_planted_neighbours_cover_every_quarter_and_state(pkg, orc):
    """Query i gets a near-duplicate ref (one coordinate one ulp off) at block i % 128, row (4 (i // 64) + i % 64) % 32: over
    the 512 queries every query residue mod 64 (the four states x 16 columns of a wave) meets all eight row quarters
    (both ref tiles x g = 0 .. 3: the owners' rows and the rows handed over by a partner), every row residue occurs."""
    m, n, k = 512, 4096, 128
    _require_lazy16(pkg, m, n, k)
    q, r = _uniform(pkg, m, n, k, 1700)
    i = np.arange(m)
    rows = (4 * (i // 64) + i % 64) % 32
    j = 32 * (i % 128) + rows
    assert np.unique(j).size == m and set(rows) == set(range(32))
    assert {(c, qr) for c, qr in zip(i % 64, rows // 4)} == {(c, qr) for c in range(64) for qr in range(8)}
    r[j] = q
    for t in range(m):
        r[j[t], t % k] = _ulp_up(r[j[t], t % k])
    _, idx, dist, _ = _search(pkg, q, r)
    assert np.array_equal(idx, j), np.nonzero(idx != j)[0][:8]
    _check_vs_v0(orc, q, r, idx, dist)


def test_lazy16_ties_over_the_four_lane_quarters(pkg, orc):
    """Eight exact copies of a query's nearest ref in one 32-ref block, two in each lane quarter (rows 1, 6, 9, 14 of ref
    tile 0 and 17, 22, 27, 30 of tile 1): whichever lanes record them, the answer is V0's — the lowest index."""
    m, n, k = 512, 4096, 128
    _require_lazy16(pkg, m, n, k)
    q, r = _uniform(pkg, m, n, k, 1800)
    copies = np.array([1, 6, 9, 14, 17, 22, 27, 30])
    assert sorted((copies % 16) // 4) == [0, 0, 1, 1, 2, 2, 3, 3]
    group = np.array([3, 64 + 19, 128 + 37, 192 + 60, 448 + 8, 500])       # all four states, several waves
    blocks = np.array([0, 17, 63, 64, 100, 127])
    for g, b in zip(group, blocks):
        r[32 * b + copies] = q[g]
    _, idx, dist, st = _search(pkg, q, r)
    assert np.array_equal(idx[group], 32 * blocks + 1), idx[group]
    assert (dist[group] == 0).all()
    _check_vs_v0(orc, q, r, idx, dist)


def test_lazy16_monotone_stream_wraps_the_lists(pkg, orc):
    """64 identical queries (one wave: every state and column) and refs at strictly decreasing distance: every tile is
    flagged and refined and every score is a record, so an owner's list takes 128 records per 256-ref stream (its own
    rows and its partner's) and wraps its 64 entries.  First half: the refs approach along the diagonal from far away —
    the entries a list wraps over lie above the threshold by then and may go; it also keeps the centred norms, hence the
    margin, large.  Second half: all refs within the margin of the last one — a wrap would drop an entry K5 needs, so
    the overflow bit sends the queries to the exact scan.  Keys are V0's: the last ref."""
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
    assert d[h] - d[-1] < 0.25 * c0, (d[h], d[-1], c0)     # the second half lies well within the margin of the last ref
    _, idx, dist, st = _search(pkg, q, r)
    assert (idx == n - 1).all(), idx
    assert st["ambiguous"] == m, st                      # every query overflowed a list: answered by the exact scan
    _check_vs_v0(orc, q, r, idx, dist)


@pytest.mark.parametrize("t_row", [5, 21])
def test_lazy16_true_nearest_ref_in_a_partner_quarter_needs_the_bound(pkg, orc, t_row):
    """test_true_nearest_ref_needs_the_bound's construction at (512, 8192, 128), per-ref records: the true nearest ref T
    (hi-midpoint values: its finished score lies ~2^-6 |x'||y'| below its hi-hi score) sits in a row quarter whose lane
    owns no list (rows 4-7 of ref tile 0, or 20-23: tile 1), behind a ref E, farther by less than that, in an owner's
    quarter (row 2) of the block before it in the same 64-ref stream.  In numpy first: T's hi-hi score is above the
    threshold E leaves, so only fl(thr + B) flags T's tile, in a lane that then hands T to its partner's list."""
    m, n, k = 512, 8192, KT
    p = _require_lazy16(pkg, m, n, k)
    assert p["slots_per_split"] == 1 and p["slot_pts"] == 64, p
    rng = np.random.default_rng(99)
    half = (rng.integers(-2 ** 15, 2 ** 15, (n // 2, k)) * 2.0 ** -16).astype(np.float32)
    mid = np.float32(1.0 + 2.0 ** -8)
    qg = np.full(k, mid, np.float32)
    T = qg.copy()
    E = (qg + np.float32(2.0 ** -4) * np.where(np.arange(k) % 2 == 0, 1, -1)).astype(np.float32)
    jE, jT = 64 * 10 + 2, 64 * 10 + 32 + t_row         # one stream: blocks 20 and 21
    half[jE], half[jT] = E, T
    r = np.concatenate([half, -half]).astype(np.float32)
    q = rng.random((m, k), dtype=np.float32) - np.float32(0.5)
    grp = np.arange(128, 128 + 64)                     # one wave: every state and column
    q[grp] = qg
    d = lambda t: t.astype(np.float64)   # noqa: E731
    X2 = float((d(qg) ** 2).sum())
    ymax2 = float((d(r) ** 2).sum(1).max())
    qh, ql = _split(qg)

    def scores(y):
        vh, vl = _split((np.float32(-2) * y).astype(np.float32))
        s_hh = float((d(y) ** 2).sum() + d(qh) @ d(vh))
        return s_hh, s_hh + float(d(qh) @ d(vl) + d(ql) @ d(vh))
    _, s3_E = scores(E)
    shh_T, s3_T = scores(T)
    c0, c1, x2 = pkg.tau_consts(k, X2, ymax2, 3)
    acc_slack = 2 * (3 * k + 3 * (k // 16) + 2) * U * (ymax2 + 4 * np.sqrt(X2 * ymax2))   # hardware summation
    thr_E = s3_E + acc_slack + 1.002 * (c0 + c1 * max(s3_E + acc_slack + x2, 0.0)) * (1 + 4 * U)
    B = pkg.split_lazy_bound(k, X2, ymax2)
    assert s3_T + acc_slack < s3_E - acc_slack                # T is the nearer one also to the filter
    assert shh_T - acc_slack > thr_E, (shh_T, thr_E)          # ... but its hi-hi score is above the threshold E leaves
    assert shh_T - s3_T <= B                                  # and B is what brings its tile back
    want_idx, want_dist = orc.v0_search(q[grp], r, threads=16)
    assert (want_idx == jT).all() and (want_dist == 0).all()
    _, idx, dist, st = _search(pkg, q, r)
    assert st["filter_form"] == "split", st
    assert np.array_equal(idx[grp], want_idx), idx[grp]
    assert np.array_equal(_bits(dist[grp]), _bits(want_dist))
