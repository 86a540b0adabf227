"""GPU tests of every MFMA filter launch configuration (FILTER_CASES of test_filter_cases_cpu.py) against the V0 oracle:
the configuration that ran is tied to the table through the index's stats, every query's distance is V0's arithmetic
on the returned ref, planted copies, split-edge refs, cross-split duplicates and near-ties plus a random sample are
checked against the oracle over all refs, and on long streams two half indices merged with keys_min reproduce every
key.  The long-stream adversarial tests run the ring-wrap and true-overflow inputs of test_gpu_parity.py on every
tile operator and tau mode whose long streams keep private thresholds (or, mixed, share them).  fp16 ("f16") and
int8 ("i8") cases run filter_f16_kernel / filter_i8_kernel: the index's filter_form ties the run to them."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_filter_cases_cpu import (FILTER_CASES, checked_queries, filter_case_id, max_planted,  # noqa: E402
                                   plan_case, refs_per_split)

pytestmark = pytest.mark.gpu

LONG_ROWS1 = [c for c in FILTER_CASES if c.key[5] and c.key[4] == "rows1"]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def v0_rows(q, r):
    """V0's arithmetic on row pairs: d = 0; for t ascending d = d + fl(q[t] - r[t])^2 in fp32 (numpy does not fuse)."""
    d = np.zeros(q.shape[0], np.float32)
    for t in range(q.shape[1]):
        diff = q[:, t] - r[:, t]
        d = d + diff * diff
    return d


def make_points(pkg, c, seed):
    """Uniform [0, 1) queries and refs (fill_uniform, the oracle's RNG bit for bit) as host fp32 arrays; bf16 and fp16
    cases hold the values the search sees (rounded to the type, widened), int8 cases the integers floor(256 u) - 128
    (uniform over -128 .. 127; at k <= 256 every V0 distance of theirs is an exact integer below 2^24)."""
    q = torch.empty((c.m, c.k), dtype=torch.float32, device="cuda")
    r = torch.empty((c.n, c.k), dtype=torch.float32, device="cuda")
    pkg.fill_uniform(q, seed, 0)
    pkg.fill_uniform(r, seed, c.m * c.k)
    if c.dtype == "bf16":
        q, r = q.to(torch.bfloat16).float(), r.to(torch.bfloat16).float()
    elif c.dtype == "f16":
        q, r = q.to(torch.float16).float(), r.to(torch.float16).float()
    elif c.dtype == "i8":
        q, r = torch.floor(q * 256.0) - 128.0, torch.floor(r * 256.0) - 128.0
    out = q.cpu().numpy(), r.cpu().numpy()
    del q, r
    return out


DEVICE_DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16, "i8": torch.int8}
FILTER_FORM = {"f16": "f16", "i8": "i8"}      # stats()["filter_form"] of the dtypes with a filter kernel of their own


def to_device(c, a):
    t = torch.from_numpy(a).cuda()
    return t.to(DEVICE_DTYPE[c.dtype]) if c.dtype in DEVICE_DTYPE else t


def open_index(pkg, c, refs_dev, index_base=0):
    return pkg.Index(refs_dev, index_base=index_base, path="mfma_perref" if c.per_ref else "mfma",
                     filter_bf16=c.dtype == "mixed")


def ulp_step(c, v, u):
    """v moved up by u units in the last place of the points' type (bf16 ulps in bf16 cases; fp16: u steps of the
    binary16 bit pattern, so a subnormal moves by one fp16 ulp too; int8: by u, towards zero where v + u leaves the
    type's range)."""
    if c.dtype == "f16":
        h = np.array([v], np.float16)
        assert h[0] == v
        return (h.view(np.uint16) + np.uint16(u)).view(np.float16).astype(np.float32)[0]
    if c.dtype == "i8":
        return np.float32(v + u if v + u <= 127 else v - u)
    b = np.array([v], np.float32).view(np.uint32)
    b = b + np.uint32(u << 16 if c.dtype == "bf16" else u)
    return b.view(np.float32)[0]


def plant(c, p, q, r, rng):
    """Plant exact copies and near-ties at positions computed from the plan.  Returns (rows, want, near_rows, dup_of):
    query rows with a known answer, that answer, the rows of near-tie queries, and {ref: its higher duplicate}."""
    n, m = c.n, c.m
    rps = refs_per_split(p)
    split_lo = [s * rps for s in range(p["splits"]) if s * rps < n]
    last_lo = split_lo[-1]
    n_near = 0 if m < 200 else min(8, max_planted(c) // 3)
    # copies: the last real ref (next to the n_pad padding), the first and last ref of every split, and a run of
    # consecutive refs (different lanes of one tile)
    run0 = min(rps // 2, max(n - 4, 0))
    targets = [n - 1, 0, min(rps, n) - 1] + list(range(run0, min(run0 + 4, n)))
    for lo in split_lo[1:]:      # (a split of one or two refs keeps one free for the duplicates below)
        targets += [lo, min(lo + rps, n) - 1] if min(lo + rps, n) - lo >= 3 else [min(lo + rps, n) - 1]
    targets = list(dict.fromkeys(targets))[:max(1, max_planted(c) - 2 * n_near)]
    used = set(targets)
    bounds = [(lo, min(lo + rps, n)) for lo in split_lo]

    def free_in(s, start, avoid_lane=None):
        """The first unused ref of split s at or after `start` (wrapping inside the split), optionally not in the
        lane (position mod 32) of ref avoid_lane; None if the split has no such ref."""
        lo, hi = bounds[s]
        for j in range(hi - lo):
            cand = lo + (start - lo + j) % (hi - lo)
            if cand not in used and (avoid_lane is None or (cand - avoid_lane) % 32 != 0):
                used.add(cand)
                return cand
        return None

    def split_of(j):
        return min(j // rps, len(bounds) - 1)

    rows = rng.permutation(m)
    ri = 0
    got_rows, got_want = [], []
    # a second identical ref at a higher index in another split (the same split when there is only one): the lower
    # index has to win through K5's merge of the splits' lists
    dup_of = {}
    for t in targets[1:3]:
        if split_of(t) != 0:
            continue
        for s in (range(1, len(bounds)) if len(bounds) > 1 else [0]):
            lo, hi = bounds[s]
            d = free_in(s, max(t + 1, lo + (hi - lo) // 3))
            if d is not None and d > t:
                r[d] = r[t]
                dup_of[t] = d
                break
    if len(bounds) > 1:
        assert dup_of and all(split_of(d) != split_of(t) for t, d in dup_of.items()), (dup_of, bounds)
    for t in targets:
        if ri >= m:
            break
        q[rows[ri]] = r[t]
        got_rows.append(rows[ri])
        got_want.append(t)
        ri += 1
    # near-ties: b is a with one coordinate moved 1-4 ulp, a and b in different splits and lanes, the query is a plus
    # noise of an ulp in three coordinates — V0's answer depends on fp32 rounding
    near_rows = []
    for i in range(n_near):
        if ri >= m:
            break
        ia = free_in(0, rps // 4 + 11 * i)
        ib = None
        others = [1 + (i + s) % (len(bounds) - 1) for s in range(len(bounds) - 1)] if len(bounds) > 1 else [0]
        for sb in (others if ia is not None else []):
            ib = free_in(sb, bounds[sb][0] + (bounds[sb][1] - bounds[sb][0]) // 5 + 11 * i + 1, avoid_lane=ia)
            if ib is not None:
                break
        if ib is None:
            continue
        assert (len(bounds) == 1 or split_of(ia) != split_of(ib)) and (ib - ia) % 32 != 0, (ia, ib, bounds)
        a = r[ia].copy()
        b = a.copy()
        cc = i % c.k
        b[cc] = ulp_step(c, b[cc], 1 + i % 4)
        r[ib] = b
        x = a.copy()
        for t in (i % c.k, (i * 7 + 3) % c.k, (i * 13 + 5) % c.k):
            x[t] = ulp_step(c, x[t], 1)
        q[rows[ri]] = x
        near_rows.append(rows[ri])
        ri += 1
    assert n_near == 0 or near_rows, "no near-tie could be planted"
    return np.array(got_rows, np.int64), np.array(got_want, np.int32), np.array(near_rows, np.int64), dup_of


@pytest.mark.timeout(600)
@pytest.mark.parametrize("c", FILTER_CASES, ids=[filter_case_id(c) for c in FILTER_CASES])
def test_filter_configuration_vs_oracle(pkg, orc, c):
    p = plan_case(pkg, c)
    rng = np.random.default_rng(c.k * 7919 + c.m * 31 + c.n)
    q, r = make_points(pkg, c, 500 + c.k)
    rows, want_rows, near_rows, dup_of = plant(c, p, q, r, rng)
    q_dev, r_dev = to_device(c, q), to_device(c, r)
    ix = open_index(pkg, c, r_dev)
    keys = ix.search_keys(q_dev)
    idx, dist = pkg.keys_unpack(keys, return_distances=True)
    torch.cuda.synchronize()
    st = ix.stats()
    near = ix.near_ties()
    ix.close()
    # the configuration that ran is the case's
    assert st["path"] == 2 and st["k_tile"] == p["kt"] and st["splits"] == p["splits"], (st, p)
    if c.dtype in FILTER_FORM:
        assert st["filter_form"] == FILTER_FORM[c.dtype], st
    assert st["nonfinite"] == 0, st
    # the filter decided: the exact scan answered at most 5 % of the queries (none when m < 20)
    assert st["ambiguous"] <= c.m // 20, st
    if near_rows.size:
        assert st["multi_candidate"] > 0, st
    # every query: an index in range and V0's distance to it, bit for bit
    idx_h, dist_h = idx.cpu().numpy(), dist.cpu().numpy()
    assert idx_h.min() >= 0 and idx_h.max() < c.n
    assert np.array_equal(_bits(v0_rows(q, r[idx_h])), _bits(dist_h))
    # planted copies: distance +0 at the lowest index holding the copy
    assert np.array_equal(idx_h[rows], want_rows), (rows, idx_h[rows], want_rows, dup_of)
    assert (dist_h[rows] == 0).all()
    # against the oracle over all refs: planted rows, a random sample and the near-tie queries
    sample, near_cap = checked_queries(c, rows.size + near_rows.size)
    tie_rows = near if near.size <= near_cap else np.random.default_rng(1).choice(near, near_cap, replace=False)
    sel = np.unique(np.concatenate([rows, near_rows, rng.choice(c.m, sample, replace=False), tie_rows]))
    want_idx, want_dist = orc.v0_search(q[sel], r, threads=16)
    bad = np.nonzero(idx_h[sel] != want_idx)[0]
    assert bad.size == 0, f"{bad.size} of {sel.size} index mismatches, first queries {sel[bad[:5]]}"
    assert np.array_equal(_bits(dist_h[sel]), _bits(want_dist))
    # long streams: two half indices (planned differently) merged with keys_min reproduce every key
    if c.key[5]:
        h = c.n // 2
        k0 = open_index(pkg, c, r_dev[:h])
        a = k0.search_keys(q_dev).clone()
        torch.cuda.synchronize()
        k0.close()
        k1 = open_index(pkg, c, r_dev[h:], index_base=h)
        b = k1.search_keys(q_dev)
        pkg.keys_min(a, b)
        torch.cuda.synchronize()
        k1.close()
        assert torch.equal(a, keys)


def _adversarial(pkg, orc, c, q, r, group):
    """Search with the case's path; (idx, stats) after checking the group and 64 random queries against the oracle
    and every query's distance against V0's arithmetic on its answer."""
    p = plan_case(pkg, c)
    ix = open_index(pkg, c, to_device(c, r))
    idx, dist = ix.search(to_device(c, q), return_distances=True)
    torch.cuda.synchronize()
    st = ix.stats()
    ix.close()
    assert st["path"] == 2 and st["k_tile"] == p["kt"] and st["splits"] == p["splits"] and st["nonfinite"] == 0, st
    if c.dtype in FILTER_FORM:
        assert st["filter_form"] == FILTER_FORM[c.dtype], st
    idx_h, dist_h = idx.cpu().numpy(), dist.cpu().numpy()
    assert idx_h.min() >= 0 and idx_h.max() < c.n
    assert np.array_equal(_bits(v0_rows(q, r[idx_h])), _bits(dist_h))
    sel = np.unique(np.concatenate([group, np.random.default_rng(2).choice(c.m, 64, replace=False)]))
    want_idx, want_dist = orc.v0_search(q[sel], r, threads=16)
    assert np.array_equal(idx_h[sel], want_idx), np.nonzero(idx_h[sel] != want_idx)[0][:5]
    assert np.array_equal(_bits(dist_h[sel]), _bits(want_dist))
    return idx_h, st


def _as_points(c, orc, a):
    if c.dtype == "f16":
        return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)
    return orc.round_bf16(a) if c.dtype == "bf16" else np.ascontiguousarray(a, np.float32)


def _four_squares(limit):
    """[limit][4]: row v holds four integers whose squares sum to v (Lagrange)."""
    s = int(np.sqrt(limit)) + 1
    a, b, cc, d = np.meshgrid(*[np.arange(s)] * 4, indexing="ij")
    tot = (a * a + b * b + cc * cc + d * d).ravel()
    out = np.zeros((limit, 4), np.int64)
    vals, first = np.unique(tot, return_index=True)
    keep = vals < limit
    assert keep.sum() == limit
    out[vals[keep]] = np.stack([x.ravel()[first[keep]] for x in (a, b, cc, d)], axis=1)
    return out


def _i8_line(pkg, c, p, q, r, G, rng):
    """The ring-wrap input for int8 points, written into q and r; returns the group's query rows.  L = 8192 refs at the
    head of the stream whose squared distances D_j to an integer centre fall strictly from 3e5 to 1e3 (a random ref
    lies at ~1e4 k): D_j = 1e3 + 2.99e5 sqrt(1 - j / (L - 1)), steps of ~18 at the far end and thousands at the near
    end, so that only the last few line refs lie within 2 tau (tau ~ 10^2) of the final minimum.  Ref j is the
    centre plus offsets of magnitude b or b + 1 in k - 8 coordinates (b^2 (k - 8) <= D_j) and, in four more, the
    four squares that make up the rest: D_j exactly, signs at random.  The last four coordinates stay at the centre's
    values: the group's queries are the centre with +-1 noise there, so every query sees D_j plus a constant.  The
    centre is small (|v| <= 16), the line's norms stay below the cloud's largest (checked) and tau does not grow."""
    L, d_hi, d_lo, k = 8192, 300000, 1000, c.k
    perm = rng.permutation(k)
    still, four, free = perm[:4], perm[4:8], perm[8:]
    kf = free.size
    centre = rng.integers(-16, 17, k).astype(np.float32)
    target = d_lo + np.rint((d_hi - d_lo) * np.sqrt(np.linspace(1.0, 0.0, L))).astype(np.int64)
    assert (np.diff(target) < 0).all()
    b = np.floor(np.sqrt(target // kf)).astype(np.int64)
    assert (b * b * kf <= target).all() and ((b + 1) ** 2 * kf > target).all()
    rem = target - kf * b * b
    nb = rem // (2 * b + 1)                     # coordinates at b + 1 (< kf), rotated from ref to ref
    rem = rem - nb * (2 * b + 1)                # 0 .. 2 b: the four squares
    off = np.zeros((L, k), np.int64)
    off[:, free] = b[:, None] + ((np.arange(kf)[None, :] + np.arange(L)[:, None]) % kf < nb[:, None])
    off[:, four] = _four_squares(int(rem.max()) + 1)[rem]
    assert np.array_equal((off * off).sum(axis=1), target) and not off[:, still].any()
    line = centre + np.where(rng.random((L, k)) < 0.5, -1, 1) * off
    assert line.min() >= -128 and line.max() <= 127
    r[:L] = line
    norm2 = (r.astype(np.float64) ** 2).sum(axis=1)
    assert norm2[:L].max() <= norm2[L:].max()
    group = rng.choice(c.m, G, replace=False)
    noise = np.zeros((G, k), np.float32)
    noise[:, still] = rng.integers(-1, 2, (G, 4))
    q[group] = centre + noise
    r64 = r.astype(np.float64)
    for g in group:
        d = v0_rows(np.repeat(q[g][None, :], L, axis=0), r[:L])
        assert (np.diff(d) <= 0).all(), "a line ref is not a record for the group"
        assert (np.diff(d) < 0).mean() > 0.9
        # fewer than half a ring of line refs within 2 tau of the query's final minimum (tau mode 1, OpI8's): the rings
        # hold what the margin keeps, and wrap on the records
        x = q[g].astype(np.float64)
        dall = norm2 - 2.0 * (r64 @ x) + x @ x
        c0, c1, x2 = pkg.tau_consts(p["kt"], float(x @ x), float(norm2.max()), 1)
        tau = c0 + c1 * max(dall.min() - x @ x + x2, 0.0)
        assert (dall[:L] <= dall.min() + 2.0 * tau).sum() < 32, tau
    return group


@pytest.mark.timeout(300)
@pytest.mark.parametrize("c", LONG_ROWS1, ids=[filter_case_id(c) for c in LONG_ROWS1])
def test_long_stream_ring_lists_wrap(pkg, orc, c):
    """Refs marching towards a group of 32 queries at the head of a long stream: every one is a new record for the
    group's lists, so the 64-entry candidate rings wrap (test_filter_sorted_refs_ring_lists on a long stream).  Parity
    holds, and the exact scan does not have to answer the whole group.  Ref j is the group's centre moved by s_j along
    axis j mod k, s_j falling from 6 to 1: the norms stay near the cloud's (tau does not grow) and bf16 rounding keeps
    the refs distinct (equal s_j on different axes are ties, not copies).  Mixed mode's margin (~2^-6 |x||y|) would
    hold most of such a line: there 2048 refs start at the cloud's centre and run from 0.9 to 0.45 of its centred ref
    norm, so the line does not raise the largest norm and the records within tau of the minimum stay below a ring per
    list.  The line comes first in the split's stream, and the host checks that each of its refs is at least as near
    to every group query as all before it: each is a record whatever lane or list it falls to.  fp16 points take the
    bf16 line rounded to binary16; int8 points an integer line of their own (_i8_line)."""
    p = plan_case(pkg, c)
    assert p["splits"] == 1
    rng = np.random.default_rng(c.k + 13)
    q, r = make_points(pkg, c, 600 + c.k)
    G = 32
    if c.dtype == "i8":
        group = _i8_line(pkg, c, p, q, r, G, rng)
        _, st = _adversarial(pkg, orc, c, q, r, group)
        assert st["ambiguous"] < G, st
        return
    if c.dtype == "mixed":      # (the margin's norms are taken about the refs' centre, ~0.5 in every coordinate)
        L, R = 2048, np.sqrt(c.k / 12.0)
        s_hi, s_lo, centre = 0.9 * R, 0.45 * R, 0.5
    else:
        L, s_hi, s_lo, centre = 8192, 6.0, 1.0, 0.125
    base = np.full(c.k, centre, np.float32)
    line = np.repeat(base[None, :], L, axis=0)
    line[np.arange(L), np.arange(L) % c.k] += np.linspace(s_hi, s_lo, L, dtype=np.float32)
    r[:L] = _as_points(c, orc, line)
    group = rng.choice(c.m, G, replace=False)
    # (bf16 rounds the noise away: the group is 32 copies of the centre.  binary16's grid is 2^-14 just below 0.125, where
    #  noise of 1e-5 would now and then move a coordinate by 6e-5 and break a tie between equal steps the wrong way
    #  round; a tenth of it leaves fp16 groups at the centre too)
    q[group] = _as_points(c, orc, base + rng.normal(0, 1e-6 if c.dtype == "f16" else 1e-5, (G, c.k)))
    for g in group:
        d = v0_rows(np.repeat(q[g][None, :], L, axis=0), r[:L])
        assert (np.diff(d) <= 0).all(), "a line ref is not a record for the group"
    _, st = _adversarial(pkg, orc, c, q, r, group)
    assert st["ambiguous"] < G, st


LONG_MIXED = [c for c in LONG_ROWS1 if c.dtype == "mixed"]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("c", LONG_MIXED, ids=[filter_case_id(c) for c in LONG_MIXED])
def test_long_stream_mixed_margin_covers_coherent_rounding(pkg, orc, c):
    """The mixed-mode margin against the operand rounding it bounds, on a long stream.  Query x is an exact copy of ref
    a; ref b, 1024 refs earlier in the same lane stream, is a hair farther.  Every centred coordinate of x and a lies
    just below a bf16 rounding midpoint (1 + 2^-8 - 2^-12, signs per pair) and b's just above it, so the bf16 operands
    make x.a too small by ~2^-7 |x||a| and leave x.b about right: the filter scores a worse than b by about half of
    tau.  A margin at a quarter of its value drops a behind b's threshold and answers b; the real one keeps both and
    K5 re-ranks to a.  The host models the bf16 scores and tau (nns_tau_consts) to keep the input that sharp."""
    p = plan_case(pkg, c)
    assert p["splits"] == 1
    rng = np.random.default_rng(c.k + 29)
    q, r = make_points(pkg, c, 800 + c.k)
    G = 8
    lo_t, hi_t = np.float32(1 + 2.0 ** -8 - 2.0 ** -12), np.float32(1 + 2.0 ** -8 + 2.0 ** -12)
    signs = np.where(rng.random((G, c.k)) < 0.5, -1.0, 1.0).astype(np.float32)
    jb = 4096 + 3 * np.arange(G)
    ja = jb + 1024
    group = rng.choice(c.m, G, replace=False)
    mean = r.astype(np.float64).mean(axis=0).astype(np.float32)
    for _ in range(2):          # the pairs move the refs' mean (K2's centre) a little: place them against the new one
        r[ja] = mean + signs * lo_t
        r[jb] = mean + signs * hi_t
        mean = (r.astype(np.float64).sum(axis=0) / c.n).astype(np.float32)
    q[group] = r[ja]
    # host model of the filter's scores |y'|^2 - 2 bf16(x').bf16(y') and of its margin at b's score
    cen = r - mean
    ymax2 = np.float32((cen.astype(np.float64) ** 2).sum(axis=1).max())
    for i, g in enumerate(group):
        xb = orc.round_bf16(q[g] - mean).astype(np.float64)
        score = {}
        for j in (ja[i], jb[i]):
            y = cen[j].astype(np.float64)
            score[j] = (y * y).sum() - 2.0 * (xb * orc.round_bf16(cen[j]).astype(np.float64)).sum()
        c0, c1, x2 = pkg.tau_consts(p["kt"], float(((q[g] - mean).astype(np.float64) ** 2).sum()), float(ymax2), 2)
        tau = c0 + c1 * max(score[jb[i]] + x2, 0.0)
        gap = score[ja[i]] - score[jb[i]]
        assert 0.35 * tau < gap < 0.75 * tau, (gap, tau)
    idx_h, st = _adversarial(pkg, orc, c, q, r, group)
    assert (idx_h[group] == ja).all(), (idx_h[group], ja)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("c", LONG_ROWS1, ids=[filter_case_id(c) for c in LONG_ROWS1])
def test_long_stream_true_overflow_falls_back(pkg, orc, c):
    """8192 exact copies of the nearest ref inside one long stream: every lane list holds more than 64 live
    candidates, the overflow bit sends the group's queries to the exact scan, and the answer is the lowest copy
    (test_filter_true_list_overflow_falls_back on a long stream).  The group's queries are the hot ref plus noise of a
    few units in the last place: 1e-3 rounded to binary16 for fp16 points, +-1 in up to four coordinates for int8."""
    rng = np.random.default_rng(c.k + 17)
    q, r = make_points(pkg, c, 700 + c.k)
    D, G = 8192, 24
    j0 = c.n // 3 + 5
    if c.dtype == "i8":
        hot = rng.integers(-128, 128, (1, c.k)).astype(np.float32)
    else:
        hot = _as_points(c, orc, rng.random((1, c.k)))
    r[j0:j0 + D] = hot
    group = rng.choice(c.m, G, replace=False)
    if c.dtype == "i8":         # the group: the hot ref moved by 1 in up to four coordinates, towards zero
        near = np.repeat(hot, G, axis=0)
        for g in range(G):
            t = rng.choice(c.k, 4, replace=False)
            near[g, t] -= np.sign(near[g, t]) * rng.integers(0, 2, 4)
        q[group] = near
    else:
        noise = {"bf16": 1e-2, "f16": 1e-3}.get(c.dtype, 1e-4)
        q[group] = _as_points(c, orc, hot + rng.normal(0, noise, (G, c.k)))
    idx_h, st = _adversarial(pkg, orc, c, q, r, group)
    assert (idx_h[group] == j0).all(), idx_h[group]
    assert st["ambiguous"] >= G, st
