"""GPU tests of the lazy split filter's refinement path (filter_lazy_kernel at KT = 128, where a query's two lanes share
their threshold: NNS_F_LAZY_SHARE) on the forced MFMA path with the lazy schedule planned.  They hold for any schedule
of the refinements, synchronous or deferred.  (There is no NNS_F_LAZY_DEFER: deferred refinements were not built, DESIGN
"Where the lazy kernel's time goes"; the file keeps the name its issue gave it.)
Every case requires, for EVERY query, V0's distance bits on the returned ref, the oracle's answer over all refs for the
case's group and a random sample, and keys equal to those of an index opened with filter_split_eager=True.  The inputs
aim at the flagged branch: every tile flagged (a refinement behind every tile), lists beyond their capacity, the end of
a stream and the lagging half block behind it, streams of one, two and AHEAD slots, a query's two lanes holding the
nearest ref and a near-tie, and the nearest ref at a split edge."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_filter_cases_cpu import ORACLE_BUDGET, refs_per_split  # noqa: E402
from test_filter_configs_gpu import _bits, v0_rows  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 128
LONG1 = (131072, 65537)     # one ref range of 2049 tiles: private thresholds by plan, per-score records
LONG2 = (65536, 140001)     # two ref ranges, long streams


def _ahead():
    src = open(os.path.join(ROOT, "nns-cuda_amd", "csrc", "filter_mfma.hip")).read()
    return int(re.search(r"#define NNS_F_LAZY_AHEAD (\d+)", src).group(1))


def _points(pkg, m, n, k, seed):
    q = torch.empty((m, k), dtype=torch.float32, device="cuda")
    r = torch.empty((n, k), dtype=torch.float32, device="cuda")
    pkg.fill_uniform(q, seed, 0)
    pkg.fill_uniform(r, seed, m * k)
    out = q.cpu().numpy(), r.cpu().numpy()
    del q, r
    return out


def _plan(pkg, m, n, k=K, per_ref=False):
    p = pkg.plan_filter(k, m, n, flags=pkg.NNS_RECORDS_PER_REF if per_ref else 0, schedule=True)
    assert p["lazy"] == 1 and p["kt"] == 128 and p["tile_rec"] == 0, p
    return p


def _search_and_check(pkg, orc, q, r, group, per_ref=False, sample=64):
    """Lazy (default) and eager-split indices on the forced MFMA path: keys equal; every query's distance is V0's
    arithmetic on its answer; the group and a random sample agree with the oracle over all refs.  (idx, stats)."""
    m, n, k = q.shape[0], r.shape[0], q.shape[1]
    sel = np.unique(np.concatenate([np.asarray(group, np.int64), np.random.default_rng(2).choice(m, min(m, sample), replace=False)]))
    assert sel.size * n * k <= ORACLE_BUDGET
    path = "mfma_perref" if per_ref else "mfma"
    q_dev, r_dev = torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda()
    got = {}
    for name, kw in (("lazy", {}), ("eager", {"filter_split_eager": True})):
        ix = pkg.Index(r_dev, path=path, **kw)
        got[name] = ix.search_keys(q_dev).clone()
        torch.cuda.synchronize()
        st = ix.stats()
        ix.close()
        assert st["path"] == 2 and st["filter_form"] == "split" and st["k_tile"] == 128 and st["nonfinite"] == 0, (name, st)
        if name == "lazy":
            st_lazy = st
    assert torch.equal(got["lazy"], got["eager"])
    idx, dist = pkg.keys_unpack(got["lazy"], return_distances=True)
    idx_h, dist_h = idx.cpu().numpy(), dist.cpu().numpy()
    assert idx_h.min() >= 0 and idx_h.max() < n
    assert np.array_equal(_bits(v0_rows(q, r[idx_h])), _bits(dist_h))
    want_idx, want_dist = orc.v0_search(q[sel], r, threads=16)
    assert np.array_equal(idx_h[sel], want_idx), sel[np.nonzero(idx_h[sel] != want_idx)[0][:5]]
    assert np.array_equal(_bits(dist_h[sel]), _bits(want_dist))
    return idx_h, st_lazy


@pytest.mark.timeout(300)
def test_every_tile_flags_for_one_wave(pkg, orc):
    """Refs marching toward the 64 queries of one wave (both of its lane states) at the head of a long stream: each of
    the first 8192 refs is nearer to every group query than all before it, so every one of the first 256 tiles is
    flagged in both states: a refinement behind every tile, each against thresholds the previous one just moved."""
    m, n = LONG1
    p = _plan(pkg, m, n)
    assert p["splits"] == 1 and p["share_thr"] == 0, p
    q, r = _points(pkg, m, n, K, 4100)
    L = 8192
    base = np.full(K, 0.125, np.float32)
    line = np.repeat(base[None, :], L, axis=0)
    line[np.arange(L), np.arange(L) % K] += np.linspace(6.0, 1.0, L, dtype=np.float32)
    r[:L] = line
    group = 64 * 777 + np.arange(64)      # (a wave carries 64 consecutive queries)
    q[group] = base + np.random.default_rng(5).normal(0, 1e-5, (64, K)).astype(np.float32)
    for g in group[::9]:
        d = v0_rows(np.repeat(q[g][None, :], L, axis=0), r[:L])
        assert (np.diff(d) <= 0).all(), "a line ref is not a record for the group"
    _, st = _search_and_check(pkg, orc, q, r, group)
    assert st["ambiguous"] < 64, st


@pytest.mark.timeout(300)
def test_copies_beyond_the_list_capacity_reach_the_exact_scan(pkg, orc):
    """8192 exact copies of the nearest ref in one long stream: the lists overflow, the overflow bit survives the
    refinement path and the group's queries are answered by the exact scan with the lowest copy."""
    m, n = LONG2
    _plan(pkg, m, n)
    rng = np.random.default_rng(17)
    q, r = _points(pkg, m, n, K, 4200)
    D, G = 8192, 24
    hot = rng.random((1, K)).astype(np.float32)
    j0 = n // 3 + 5
    r[j0:j0 + D] = hot
    group = rng.choice(m, G, replace=False)
    q[group] = (hot + rng.normal(0, 1e-4, (G, K))).astype(np.float32)
    idx_h, st = _search_and_check(pkg, orc, q, r, group)
    assert (idx_h[group] == j0).all(), idx_h[group]
    assert st["ambiguous"] >= G, st


@pytest.mark.timeout(300)
def test_only_near_ref_in_the_last_block_and_at_a_split_edge(pkg, orc):
    """Exact copies of single refs — nothing else of the uniform cloud is within tau of them — as the queries of a
    leading wave (0) and of a lagging wave (5, which retires the stream's last block in its half-block tail after the
    slot loop): in the last block of the first ref range, in the first block of the second (the two sides of the split
    edge), in the last block of the last range, and in the last block's other lane half."""
    m, n = LONG2
    p = _plan(pkg, m, n)
    assert p["splits"] == 2 and p["share_thr"] == 0, p
    rps = refs_per_split(p)
    assert 0 < rps < n
    q, r = _points(pkg, m, n, K, 4300)
    targets = [rps - 1, rps - 5, rps - 32, rps, rps + 4, n - 1, n - 2, n - 30]
    rows = []
    for i, t in enumerate(targets):
        for wave in (0, 5):
            rows.append(512 * (3 + i) + 64 * wave + (7 * i + 11 * wave) % 64)
            q[rows[-1]] = r[t]
    rows = np.array(rows)
    idx_h, st = _search_and_check(pkg, orc, q, r, rows)
    assert np.array_equal(idx_h[rows], np.repeat(targets, 2)), (idx_h[rows], targets)
    assert st["ambiguous"] <= m // 20, st      # (the filter decided, as in test_filter_configs_gpu.py)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("slots", ["one", "two", "ahead"])
def test_streams_of_one_two_and_ahead_slots(pkg, orc, slots):
    """Per-ref records with few queries: 256 ref ranges of exactly 1, 2 and AHEAD 64-ref ring slots each — shorter than,
    equal to and just beyond what the prologue has in flight; copies at the range edges, every query checked."""
    s = {"one": 1, "two": 2, "ahead": _ahead()}[slots]
    m, n = 250, 64 * 256 * s - 7
    p = _plan(pkg, m, n, per_ref=True)
    assert p["slots_per_split"] == s and p["splits"] == 256 and p["slot_pts"] == 64, p
    q, r = _points(pkg, m, n, K, 4400 + s)
    rps = refs_per_split(p)
    targets = [0, rps - 1, rps, 2 * rps - 1, 17 * rps + 31, 17 * rps + 32, n - 1]
    rows = np.arange(len(targets)) * 33 + 3
    for row, t in zip(rows, targets):
        q[row] = r[t]
    idx_h, _ = _search_and_check(pkg, orc, q, r, rows, per_ref=True, sample=m)
    assert np.array_equal(idx_h[rows], targets)


def _ulp_up(v, u):
    return (np.array([v], np.float32).view(np.uint32) + np.uint32(u)).view(np.float32)[0]


@pytest.mark.timeout(300)
def test_nearest_ref_and_near_tie_on_the_two_lanes_of_a_query(pkg, orc):
    """A query's two lanes (l and l ^ 32) see rows 0-3, 8-11, .. and rows 4-7, 12-15, .. of every 32-ref block.  The true
    nearest ref T sits in row 0 of a block (lane l) and a ref E — T with one coordinate moved 1 - 4 ulp, or an exact
    duplicate — in row 4 of another block of the same stream (lane l ^ 32), earlier or later than T.  With shared
    thresholds the second lane tests against the first one's threshold: both refs must still reach K5, whose V0
    re-rank decides between them (the duplicate: the lower index wins).  Long streams: the plan keeps share_thr 0."""
    m, n = LONG2
    p = _plan(pkg, m, n)
    assert p["share_thr"] == 0, p
    rps = refs_per_split(p)
    q, r = _points(pkg, m, n, K, 4500)
    rows, expect = [], {}
    for i in range(12):
        bT, bE = (1200 + 40 * i, 300 + 7 * i) if i % 2 else (300 + 7 * i, 1200 + 40 * i)   # E earlier / E later
        jT, jE = 32 * bT, 32 * bE + 4
        assert jT < rps and jE < rps
        T = r[jT].copy()
        E = T.copy()
        if i % 3:
            E[(5 * i) % K] = _ulp_up(E[(5 * i) % K], 1 + i % 4)
        else:
            expect[i] = min(jT, jE)     # exact duplicate
        r[jE] = E
        x = T.copy()
        for t in (i % K, (7 * i + 3) % K):
            x[t] = _ulp_up(x[t], 1)
        if not i % 3:
            x = T
        row = 512 * (5 + i) + 64 * (i % 8) + (3 * i) % 32 + 32 * (i % 2)
        q[row] = x
        rows.append(row)
    rows = np.array(rows)
    idx_h, st = _search_and_check(pkg, orc, q, r, rows)
    for i, want in expect.items():
        assert idx_h[rows[i]] == want, (i, idx_h[rows[i]], want)
    assert st["multi_candidate"] >= len(rows), st
