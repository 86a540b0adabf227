"""GPU tests of top-K (K6) at the edges its random-cloud tests do not reach, against the numpy V0 oracle of
test_topk_cpu.py (indices exact, distances bit for bit): every scan instantiation (tile width x load width x point
type, misaligned refs included), sustained queue pressure (floods, bursts around the flush mark, ties at the cut),
the split merge's padding, rows past the unpack grid and the pair merge's 65 535-row mark, query-side specials and
extreme magnitudes, and an index's lifecycle under top-K."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_topk_cpu import SCAN_CASES, scan_case_id, scan_vec, topk_oracle  # noqa: E402
from test_topk_gpu import NONE, _assert_same, _bits  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _rand(seed, *shape):
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


def _widen(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def _as_searched(pkg, a, bf16):
    """The fp32 values a search of `a` sees (bf16: rounded to bf16 and widened)."""
    a = np.ascontiguousarray(a, np.float32)
    return _widen(pkg.to_bf16_bits(a)) if bf16 else a


def _to_dev(pkg, a, bf16):
    a = np.ascontiguousarray(a, np.float32)
    if bf16:
        return torch.from_numpy(pkg.to_bf16_bits(a).view(np.int16)).to(DEV).view(torch.bfloat16)
    return torch.from_numpy(a).to(DEV)


def _v0_all(q, r):
    """Every V0 distance [m][n] (the oracle's arithmetic, unsorted)."""
    d = np.zeros((q.shape[0], r.shape[0]), np.float32)
    with np.errstate(all="ignore"):
        for t in range(q.shape[1]):
            diff = q[:, t:t + 1] - r[None, :, t]
            d = d + diff * diff
    return d


def _whole(pkg, q, r, kn, bf16=False, **kw):
    """The whole call (fp32, or bf16 bit patterns of the rounded data) checked against the oracle."""
    q, r = _as_searched(pkg, q, bf16), _as_searched(pkg, r, bf16)
    if bf16:
        idx, dist = pkg.search_topk_bf16(pkg.to_bf16_bits(q), pkg.to_bf16_bits(r), kn, return_distances=True, **kw)
    else:
        idx, dist = pkg.search_topk(q, r, kn, return_distances=True, **kw)
    want_idx, want_dist = topk_oracle(q, r, kn)
    _assert_same(idx, dist, want_idx, want_dist,
                 f"whole call m={q.shape[0]} n={r.shape[0]} k={q.shape[1]} kn={kn} bf16={bf16} {kw}")
    return idx, dist


def _index_topk(pkg, refs, queries, kn, keys=None, **kw):
    """Keys, indices and distances of one Index top-K search (host arrays)."""
    ix = pkg.Index(refs, **kw)
    keys = ix.search_topk_keys(queries, kn, keys=keys)
    idx, dist = pkg.keys_topk_unpack(keys, return_distances=True)
    torch.cuda.synchronize()
    ix.close()
    return keys.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy()


# ---- 1. every scan instantiation -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SCAN_CASES, ids=[scan_case_id(c) for c in SCAN_CASES])
def test_every_scan_instantiation(pkg, case):
    bf16 = case.dtype == "bf16"
    k, m, n, kn = case.k, case.m, case.n, case.kn
    assert pkg.plan_topk(k, m, n, kn, bf16=bf16)["queries_per_wg"] == case.qt
    seed = 7 * k + 131 * m + kn
    q = _rand(seed, m, k) * np.float32(2) - np.float32(1)
    r = _rand(seed + 1, n, k) * np.float32(2) - np.float32(1)
    r[n // 2:n // 2 + 40] = r[3]                       # a run of equal distances for every query
    q, r = _as_searched(pkg, q, bf16), _as_searched(pkg, r, bf16)
    want_idx, want_dist = topk_oracle(q, r, kn)
    esz = 2 if bf16 else 4
    flat = _to_dev(pkg, r, bf16).reshape(-1)
    buf = torch.empty(case.offset + n * k, dtype=flat.dtype, device=DEV)
    buf[case.offset:].copy_(flat)
    view = buf[case.offset:].view(n, k)                # storage offset: the pointer may be misaligned on purpose
    assert scan_vec(k, view.data_ptr(), esz) == case.vec
    runs = [view]
    if case.vec == 1 and k % 4 == 0:
        aligned = view.clone()                         # the same data through the 4-wide loads
        assert scan_vec(k, aligned.data_ptr(), esz) == 4
        runs.append(aligned)
    qd = _to_dev(pkg, q, bf16)
    got = []
    for refs in runs:
        keys, idx, dist = _index_topk(pkg, refs, qd, kn, path="exact")
        vec = scan_vec(k, refs.data_ptr(), esz)
        _assert_same(idx, dist, want_idx, want_dist, f"{scan_case_id(case)} VEC={vec}")
        got.append(keys)
    assert all(np.array_equal(g, got[0]) for g in got)
    _whole(pkg, q, r, kn, bf16)


@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("k", [1, 3, 33, 257])
def test_bf16_odd_k_few_queries(pkg, k, m):
    n = 3000
    for kn in (1, 7, 64):
        q = _rand(900 + k + m, m, k) * np.float32(4)
        r = _rand(950 + k + m + kn, n, k) * np.float32(4)
        _whole(pkg, q, r, kn, bf16=True)


# ---- 2. queue pressure -----------------------------------------------------------------------------------------
TOP_BITS = 0x5D80   # bf16 bits of 2^60: refs take distinct bf16 values below it, so their squares are exact


def _descending_values(n, top=TOP_BITS):
    """n distinct positive values, strictly decreasing, exact in bf16 (and their squares in fp32)."""
    assert n <= top - 0x2180                              # stay above 2^-60
    return _widen(np.arange(top - 1, top - 1 - n, -1))


def _axis_points(x, k=4):
    p = np.zeros((len(x), k), np.float32)
    p[:, 0] = x
    return p


def _flood_queries(m):
    # q_u = -u * 2^-64: every ref is closer than all refs before it, for every query of the tile
    return _axis_points(-np.arange(m, dtype=np.float32) * np.float32(2.0 ** -64))


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [2000, 15360], ids=["one-split", "many-splits"])
@pytest.mark.parametrize("kn", [1, 16, 17, 255, 256])
def test_flood_every_ref_beats_the_list(pkg, kn, n, bf16):
    # every lane appends every round: the queue fills to 512 every second round and the threshold drops at every flush
    m = 16
    splits = pkg.plan_topk(4, m, n, kn, bf16=bf16)["splits"]
    assert (splits == 1) == (n == 2000), splits
    q, r = _flood_queries(m), _axis_points(_descending_values(n))
    assert np.array_equal(_as_searched(pkg, r, True), r) and np.array_equal(_as_searched(pkg, q, True), q)
    d = _v0_all(q, r)
    assert np.isfinite(d).all() and (np.diff(d, axis=1) < 0).all()
    idx, _ = _whole(pkg, q, r, kn, bf16)
    assert (idx == np.arange(n - 1, n - 1 - kn, -1)[None, :]).all()


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [2000, 15360], ids=["one-split", "many-splits"])
@pytest.mark.parametrize("kn", [16, 17, 256])
def test_flood_one_query_of_a_quiet_tile(pkg, kn, n, bf16):
    # query 3 floods; the other 15 (kn <= 16: one 16-wide tile) or 7 (two 8-wide tiles) see increasing distances
    m, loud = 16, 3
    q = _axis_points(np.full(m, 2.0 ** 61, np.float32))
    q[loud, 0] = 0.0
    r = _axis_points(_descending_values(n))
    d = _v0_all(q, r)
    assert (np.diff(d[loud]) < 0).all()
    assert (np.diff(np.delete(d, loud, axis=0), axis=1) >= 0).all()
    idx, _ = _whole(pkg, q, r, kn, bf16)
    assert (idx[loud] == np.arange(n - 1, n - 1 - kn, -1)).all()


# refs per 256-ref round that beat everything before them (the rest are far).  One split (kn = 256) ends its rounds
# with queue counts 256 | 512 F | 255 | 256 | 257 F | 256 | 512 F | 57 | 313 F | 256 | 456 F | 56 | 56 | 57 | 256 |
# 257 F (F: flushed); with kn <= 128 the refs form two splits of 8 rounds, the second starting with an empty list.
BURSTS = [256, 1, 255, 1, 1, 256, 256, 57, 256, 256, 200, 56, 0, 1, 199, 1]


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("kn", [1, 17, 256])
def test_bursts_around_the_flush_mark(pkg, kn, bf16):
    m, n = 8, 256 * len(BURSTS)
    rng = np.random.default_rng(1000 + kn)
    best = iter(_descending_values(sum(BURSTS)))
    x = _widen(rng.integers(0x5E00, 0x5E80, n))           # fillers in [2^61, 2^62): never beat a listed ref
    for rd, c in enumerate(BURSTS):
        lanes = rd * 256 + rng.choice(256, c, replace=False)
        for j in np.sort(lanes):
            x[j] = next(best)
    q, r = _flood_queries(m), _axis_points(x)
    _whole(pkg, q, r, kn, bf16)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("kn,below", [(1, 0), (16, 15), (16, 11), (17, 16), (17, 12), (256, 255), (256, 249)])
def test_ties_straddle_the_cut(pkg, kn, below, bf16):
    # `below` refs strictly nearer than D sit in the first rounds; a run of refs at exactly D (the 8 sign / swap
    # images of (1.5, 2.25) and copies) arrives in later rounds and later splits and covers slots below .. kn - 1
    # and beyond; (distance, index) order keeps its lowest indices
    k, m, n = 2, 9, 40000
    plan = pkg.plan_topk(k, m, n, kn, bf16=bf16)
    per = plan["per"]
    assert plan["splits"] > 2
    rng = np.random.default_rng(2000 + kn + below)
    r = _widen(rng.integers(0x4120, 0x41A0, (n, k)))      # far: coordinates in [10, 20)
    near = rng.choice(768, below, replace=False)          # rounds 0 .. 2 of split 0
    r[near] = 0.0
    r[near, 0] = _widen(0x3F80 - np.arange(below))         # distinct values <= 1: squares distinct and < D
    images = np.array([[a, b] for a, b in ((1.5, 2.25), (2.25, 1.5)) for a in (a, -a) for b in (b, -b)], np.float32)
    late = np.concatenate([rng.choice(np.arange(1024, per), 3, replace=False),   # split 0, after its first flushes
                           rng.choice(np.arange(per, n), kn - below + 8, replace=False)])
    r[late] = images[np.arange(len(late)) % 8]
    q = _rand(2100, m, k) * np.float32(10) + np.float32(10)
    q[0] = q[4] = 0.0
    want_idx, want_dist = topk_oracle(q, r, kn)
    assert (want_idx[0, below:] == np.sort(late)[:kn - below]).all()
    assert (want_dist[0, below:] == np.float32(7.3125)).all()
    for shards in (1, 2):
        _whole(pkg, q, r, kn, bf16, shards=shards)


# ---- 3. split merge with fewer selectable refs than kn ----------------------------------------------------------
GARBAGE = (1 << 32) | 7     # a plausible key (a tiny distance, index 7): a slot the merge fails to write shows up


@pytest.mark.parametrize("kn", [100, 256])
def test_split_merge_pads_when_few_refs_are_selectable(pkg, kn):
    k, m, n = 2, 9, 1 << 18
    plan = pkg.plan_topk(k, m, n, kn)
    per, splits = plan["per"], plan["splits"]
    assert splits > 2
    rng = np.random.default_rng(3000 + kn)
    r = rng.random((n, k), dtype=np.float32)
    spoil = np.array([np.nan, np.inf, -np.inf, 3e19], np.float32)   # 3e19: the square overflows to +INF
    r[np.arange(n), rng.integers(0, k, n)] = spoil[np.arange(n) % 4]
    first = rng.choice(per, 40, replace=False)
    last = (splits - 1) * per + rng.choice(n - (splits - 1) * per, 30, replace=False)
    ok = np.concatenate([first, last])
    r[ok] = rng.random((len(ok), k), dtype=np.float32)   # only the first and the last split hold selectable refs
    q = rng.random((m, k), dtype=np.float32)
    q[2, 1] = np.nan                                     # a row with nothing selectable at all
    # the whole call's buffers come from the library's pool: leave valid keys of this shape in them first
    pkg.search_topk(np.nan_to_num(q), rng.random((n, k), dtype=np.float32), kn)
    for bf16 in (False, True):
        idx, dist = _whole(pkg, q, r, kn, bf16)
        assert (idx[:, 70:] == -1).all() and np.isinf(dist[:, 70:]).all()
        assert (idx[2] == -1).all()
        assert (np.delete(idx, 2, axis=0)[:, :70] >= 0).all()
    want_idx, want_dist = topk_oracle(q, r, kn)
    keys = torch.full((m, kn), GARBAGE, dtype=torch.int64, device=DEV)
    got, idx, dist = _index_topk(pkg, torch.from_numpy(r).to(DEV), torch.from_numpy(q).to(DEV), kn, keys=keys,
                                 path="exact")
    _assert_same(idx, dist, want_idx, want_dist, "index path")
    assert (got[:, 70:] == NONE).all() and (got[2] == NONE).all()


# ---- 4. rows past the unpack grid and the pair merge's 65 535-row mark -------------------------------------------
def test_big_rows_unpack_stride_and_pair_merge(pkg):
    k, m, n, kn = 2, 65600, 300, 256
    assert m * kn > 65536 * 256 and m > 65535     # unpack strides; the merges' grid.x passes 65 535
    q, r = _rand(4000, m, k), _rand(4001, n, k)
    r[200:230] = r[10]
    want_idx, want_dist = topk_oracle(q, r, kn)
    idx, dist = pkg.search_topk(q, r, kn, return_distances=True)
    _assert_same(idx, dist, want_idx, want_dist, "whole call")
    del idx, dist
    rt, qd = torch.from_numpy(r).to(DEV), torch.from_numpy(q).to(DEV)
    half = 150
    a = pkg.Index(rt[:half], path="exact")
    b = pkg.Index(rt[half:], index_base=half, path="exact")
    ka = a.search_topk_keys(qd, kn)
    kb = b.search_topk_keys(qd, kn)
    pkg.keys_topk_merge(ka, kb)
    idx, dist = pkg.keys_topk_unpack(ka, return_distances=True)
    torch.cuda.synchronize()
    _assert_same(idx.cpu().numpy(), dist.cpu().numpy(), want_idx, want_dist, "merged halves")
    a.close()
    b.close()


# ---- 5. keys_topk_merge against numpy ---------------------------------------------------------------------------
@pytest.mark.parametrize("kn", [1, 2, 63, 64, 65, 128, 255, 256])
def test_keys_topk_merge_random_rows(pkg, kn):
    rng = np.random.default_rng(5000 + kn)
    m = 300
    la, lb = rng.integers(0, kn + 1, m), rng.integers(0, kn + 1, m)
    la[:4], lb[:4] = [0, kn, 0, kn], [0, kn, kn, 0]       # both empty, both full, one of each
    dvals = _bits(np.array([0.0, 1e-45, 0.5, 0.5000001, 1.0, 3.4e38], np.float32)).astype(np.int64)
    a = np.full((m, kn), NONE, np.int64)
    b = np.full((m, kn), NONE, np.int64)
    want = np.full((m, kn), NONE, np.int64)
    for i in range(m):
        cnt = la[i] + lb[i]
        ids = rng.choice(1 << 20, cnt, replace=False) * 2047   # disjoint across the two rows, up to ~2^31
        keys = (rng.choice(dvals, cnt) << 32) | ids          # few distances: equal ones within and across rows
        a[i, :la[i]] = np.sort(keys[:la[i]])
        b[i, :lb[i]] = np.sort(keys[la[i]:])
        both = np.sort(keys)[:kn]
        want[i, :len(both)] = both
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    pkg.keys_topk_merge(ta, tb)
    idx, dist = pkg.keys_topk_unpack(ta, return_distances=True)
    torch.cuda.synchronize()
    got = ta.cpu().numpy()
    assert np.array_equal(got, want), f"first bad row {np.argwhere((got != want).any(axis=1))[:3].ravel()}"
    assert np.array_equal(tb.cpu().numpy(), b)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    full = want != NONE
    assert (idx[~full] == -1).all() and np.isposinf(dist[~full]).all()
    assert np.array_equal(idx[full], (want[full] & 0xFFFFFFFF).astype(np.int32))
    assert np.array_equal(_bits(dist[full]), (want[full] >> 32).astype(np.uint32))


# ---- 6. specials --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_nonfinite_and_overflowing_queries(pkg, bf16):
    k, m, n, kn = 8, 32, 20000, 16
    q = _rand(6000, m, k)
    r = _rand(6001, n, k)
    bad = {1: np.nan, 4: np.inf, 6: -np.inf, 13: 3e19, 20: -3e19}
    for row, v in bad.items():
        q[row, row % k] = v
    assert pkg.plan_topk(k, m, n, kn)["splits"] > 1
    idx, dist = _whole(pkg, q, r, kn, bf16)
    rows = sorted(bad)
    assert (idx[rows] == -1).all() and np.isposinf(dist[rows]).all()
    good = [i for i in range(m) if i not in bad]
    idx2, dist2 = _whole(pkg, q[good], r, kn, bf16)      # the tile neighbours answer as without the bad rows
    _assert_same(idx[good], dist[good], idx2, dist2, "neighbours of non-finite queries")


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_signed_zeros(pkg, bf16):
    k, m, n, kn = 4, 12, 3000, 64
    rng = np.random.default_rng(6100)
    r = _rand(6101, n, k)
    zero = rng.random(n) < 0.3
    r[zero] = np.where(rng.random((int(zero.sum()), k)) < 0.5, np.float32(0.0), np.float32(-0.0))
    q = _rand(6102, m, k)
    q[:4] = np.where(rng.random((4, k)) < 0.5, np.float32(0.0), np.float32(-0.0))
    idx, dist = _whole(pkg, q, r, kn, bf16)
    assert (idx[:4] == np.flatnonzero(zero)[:kn][None, :]).all()
    assert (_bits(dist[:4]) == 0).all()                  # +0.0, never -0.0


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("scale", [1e-20, 1e-23], ids=["subnormal-squares", "squares-underflow"])
def test_subnormal_scale(pkg, scale, bf16):
    # diff^2 is subnormal (1e-20) or rounds to 0 (1e-23): an FTZ build would change the bits / the order
    k, m, n, kn = 3, 20, 5000, 64
    q = _rand(6200, m, k) * np.float32(scale)
    r = _rand(6201, n, k) * np.float32(scale)
    _, dist = _whole(pkg, q, r, kn, bf16)
    tiny = np.finfo(np.float32).tiny
    if scale == 1e-20:
        assert ((dist > 0) & (dist < tiny)).mean() > 0.9
    else:
        assert (dist == 0).mean() > 0.5                   # long runs of exact ties, ordered by index


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_distances_just_below_flt_max(pkg, bf16):
    # two terms near 1.3e19 stay finite just under FLT_MAX; a third such term overflows
    k, m, n, kn = 3, 10, 4000, 64
    rng = np.random.default_rng(6300)
    r = np.empty((n, k), np.float32)
    r[:, :2] = rng.uniform(1.27e19, 1.295e19, (n, 2))   # two squares: 3.2e38 .. 3.36e38
    r[:, 2] = rng.uniform(-1, 1, n)
    r[::5, 2] = 1.3e19
    r[1::7, :2] *= -1
    q = rng.uniform(-1e16, 1e16, (m, k)).astype(np.float32)
    q[0] = 0.0
    idx, dist = _whole(pkg, q, r, kn, bf16)
    assert np.isfinite(dist).all() and (_bits(dist) >= 0x7F700000).all()   # key high words 0x7F70.. 0x7F7F
    assert not np.isin(idx, np.arange(0, n, 5)).any()


# ---- 7. lifecycle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["exact", "auto"])
def test_dimension_major_index_refresh(pkg, path):
    k, m, n, kn = 20, 17, 30000, 40
    q = _rand(7000, m, k)
    r1, r2 = _rand(7001, n, k), _rand(7002, n, k)
    soa = torch.from_numpy(np.ascontiguousarray(r1.T)).to(DEV)
    qd = torch.from_numpy(q).to(DEV)
    ix = pkg.Index(soa, soa=True, path=path)
    for r in (r1, r2):
        if r is r2:
            soa.copy_(torch.from_numpy(np.ascontiguousarray(r2.T)))   # the caller rewrites its [k][n] array
            ix.refresh()
        idx, dist = ix.search_topk(qd, kn, return_distances=True)
        torch.cuda.synchronize()
        want_idx, want_dist = topk_oracle(q, r, kn)
        _assert_same(idx.cpu().numpy(), dist.cpu().numpy(), want_idx, want_dist, f"soa {path} refresh={r is r2}")
    ix.close()


def test_queued_searches_regrow_the_split_workspace(pkg):
    k, n = 4, 100000
    shapes = [(4, 8), (64, 256), (4, 16)]
    plans = [pkg.plan_topk(k, m, n, kn) for m, kn in shapes]
    assert all(p["splits"] > 1 for p in plans)
    assert plans[0]["ws_keys"] < plans[1]["ws_keys"] > plans[2]["ws_keys"]
    r = _rand(7100, n, k)
    qs = [_rand(7101 + i, m, k) for i, (m, _) in enumerate(shapes)]
    ix = pkg.Index(torch.from_numpy(r).to(DEV), path="exact")
    out = [ix.search_topk(torch.from_numpy(qh).to(DEV), kn, return_distances=True)   # no wait in between
           for qh, (_, kn) in zip(qs, shapes)]
    torch.cuda.synchronize()
    for qh, (_, kn), (idx, dist) in zip(qs, shapes, out):
        want_idx, want_dist = topk_oracle(qh, r, kn)
        _assert_same(idx.cpu().numpy(), dist.cpu().numpy(), want_idx, want_dist, f"queued kn={kn}")
    ix.close()


def test_index_base_at_the_int32_top(pkg):
    k, m, n, kn = 3, 12, 5000, 32
    base = 2 ** 31 - 1 - n
    r, q = _rand(7200, n, k), _rand(7201, m, k)
    q[0], q[1] = r[n - 1], r[0]
    want_idx, want_dist = topk_oracle(q, r, kn)
    want_idx = np.where(want_idx >= 0, want_idx.astype(np.int64) + base, -1).astype(np.int32)
    assert want_idx[0, 0] == 2 ** 31 - 2
    rt, qd = torch.from_numpy(r).to(DEV), torch.from_numpy(q).to(DEV)
    whole, idx, dist = _index_topk(pkg, rt, qd, kn, index_base=base, path="exact")
    _assert_same(idx, dist, want_idx, want_dist, "index at the int32 top")
    half = 2600
    a = pkg.Index(rt[:half], index_base=base, path="exact")
    b = pkg.Index(rt[half:], index_base=base + half, path="exact")
    ka = a.search_topk_keys(qd, kn)
    kb = b.search_topk_keys(qd, kn)
    pkg.keys_topk_merge(ka, kb)
    idx, dist = pkg.keys_topk_unpack(ka, return_distances=True)
    torch.cuda.synchronize()
    assert np.array_equal(ka.cpu().numpy(), whole)
    _assert_same(idx.cpu().numpy(), dist.cpu().numpy(), want_idx, want_dist, "merged halves at the int32 top")
    a.close()
    b.close()


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("shards", [1, 2])
def test_whole_call_without_distances(pkg, shards, bf16):
    k, m, n, kn = 6, 70, 20000, 50
    q, r = _rand(7300, m, k), _rand(7301, n, k)
    want, _ = _whole(pkg, q, r, kn, bf16, shards=shards)
    if bf16:
        idx = pkg.search_topk_bf16(pkg.to_bf16_bits(q), pkg.to_bf16_bits(r), kn, shards=shards)
    else:
        idx = pkg.search_topk(q, r, kn, shards=shards)
    assert np.array_equal(idx, want)
