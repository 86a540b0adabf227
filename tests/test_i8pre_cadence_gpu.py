"""GPU tests of the int8 pre-pass's barrier cadence (filter_i8pre_kernel, OpI8Pre: one workgroup barrier per G =
kI8PreGroup intervals, the waves drifting apart inside a group).  A wave's thresholds depend on its own stream alone, so
whatever the cadence the keys are those of Index(filter_i8pre="off") and V0's.  m = 512 is one workgroup of eight waves
(wave w: queries 64 w .. 64 w + 63); the plan cuts the refs into at most 256 streams, so a stream of S slots of 64 refs
takes n ~ 16384 S.  Every test asserts filter_pre()."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_filter_cases_cpu import ORACLE_BUDGET  # noqa: E402
from test_filter_configs_gpu import _bits, v0_rows  # noqa: E402
from test_lazy16_gpu import _ulp_up, _uniform  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_H = open(os.path.join(ROOT, "nns-cuda_amd", "csrc", "nns_internal.h")).read()
RING = int(re.search(r"constexpr int kI8PreRingDepth = (\d+);", _H).group(1))
AHEAD = int(re.search(r"#define NNS_F_PRE_AHEAD (\d+)", _H).group(1))
G = int(re.search(r"#define NNS_F_PRE_GROUP (\d+)", _H).group(1))
M, K = 512, 128
SLOT = 64


def _n_for(pkg, slots):
    """n, not a multiple of 64, whose plan gives every stream `slots` ring slots (the last one a padded slot)"""
    n = slots * 256 * SLOT - 27
    p = pkg.plan_filter(K, M, n, flags=pkg.NNS_RECORDS_PER_REF, schedule=True)
    assert p["lazy"] == 1 and p["kt"] == K and p["tile_rec"] == 0 and p["qgroups"] == 1, p
    assert p["slots_per_split"] == slots and p["slot_pts"] == SLOT and n % SLOT != 0, (slots, p)
    assert pkg.filter_lazy_tile() == 16
    return n, p


def _keys(pkg, ix, qd, want_pre):
    keys = ix.search_keys(qd).clone()
    torch.cuda.synchronize()
    st = ix.stats()
    assert ix.filter_pre() == want_pre, st
    assert st["path"] == 2 and st["k_tile"] == K and st["nonfinite"] == 0, st
    return keys, st


def _check(pkg, orc, q, r, group=(), sample=64, seed=3):
    """One search under the forced pre-pass and one with it off: equal keys; every distance is V0's arithmetic on its
    answer; the group and a random sample (all queries where the budget allows) agree with the oracle.  (idx, keys)"""
    m, n = q.shape[0], r.shape[0]
    if m * n * K <= ORACLE_BUDGET / 16:
        sel = np.arange(m)
    else:
        sel = np.unique(np.concatenate([np.asarray(group, np.int64), np.random.default_rng(seed).choice(m, sample, replace=False)]))
    assert sel.size * n * K <= ORACLE_BUDGET
    qd, rd = torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda()
    got = {}
    for mode, want in (("force", True), ("off", False)):
        ix = pkg.Index(rd, path="mfma_perref", filter_i8pre=mode)
        got[mode], _ = _keys(pkg, ix, qd, want)
        ix.close()
    assert torch.equal(got["force"], got["off"])
    idx, dist = pkg.keys_unpack(got["force"], return_distances=True)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    assert idx.min() >= 0 and idx.max() < n
    assert np.array_equal(_bits(v0_rows(q, r[idx])), _bits(dist))
    want_idx, want_dist = orc.v0_search(q[sel], r, threads=16)
    assert np.array_equal(idx[sel], want_idx), sel[np.nonzero(idx[sel] != want_idx)[0][:5]]
    assert np.array_equal(_bits(dist[sel]), _bits(want_dist))
    return idx, got["force"]


# ---- stream lengths around the cadence ------------------------------------------------------------------------------------
LENGTHS = sorted({s for s in (1, G - 1, G, G + 1, 2 * G, 2 * G + 1, AHEAD, AHEAD + 1, RING, RING + 1, 3 * RING + G + 1) if s >= 1})


@pytest.mark.parametrize("slots", LENGTHS)
def test_cadence_stream_lengths(pkg, orc, slots):
    """Uniform clouds, streams of `slots` slots: shorter than a group, a whole group, a last partial group, the DMA lead
    and one more, a ring turn and one more, three turns and a partial group."""
    n, _ = _n_for(pkg, slots)
    q, r = _uniform(pkg, M, n, K, 3100 + slots)
    _check(pkg, orc, q, r)


# ---- maximum drift ----------------------------------------------------------------------------------------------------
DRIFT_SLOTS = 3 * RING + 1
_drift = {}


def _drift_refs(pkg):
    """(x, z, refs).  Refs on a strictly falling line x + t_j (1, .., 1), t from 3/4 down to 1/2: to a query at x every
    ref is a new record, as in test_i8pre_monotone_stream_wraps_the_lists.  The FIRST ref of every stream is replaced by a
    copy of z, a point off the line's far end (x + 1 or x + 0.95 per coordinate; stream b's copy is 1 + b // K ulps up
    in coordinate b % K), farther from x than any ref of the line and at a squared distance of 5 or more from all of them.
    Streams of three ring turns and a slot.  Built once, not modified."""
    if not _drift:
        n, p = _n_for(pkg, DRIFT_SLOTS)
        rng = np.random.default_rng(23)
        x = (rng.random(K, dtype=np.float32) * np.float32(0.5) + np.float32(0.25)).astype(np.float32)
        t = np.linspace(0.75, 0.5, n, dtype=np.float32)
        r = (x[None, :] + t[:, None]).astype(np.float32)
        d = ((r.astype(np.float64) - x.astype(np.float64)) ** 2).sum(1)
        assert (np.diff(d) < 0).all()
        z = (x + np.where(rng.random(K) < 0.5, np.float32(1.0), np.float32(0.95)).astype(np.float32)).astype(np.float32)
        dz = ((r[::499].astype(np.float64) - z.astype(np.float64)) ** 2).sum(1)
        assert dz.min() > 5.0 and ((z.astype(np.float64) - x) ** 2).sum() > d.max() + 5.0
        for b in range(p["splits"]):
            j = b * DRIFT_SLOTS * SLOT
            if j < n:
                r[j] = z
                for _ in range(1 + b // K):
                    r[j, b % K] = _ulp_up(r[j, b % K])
        _drift["x"], _drift["z"], _drift["r"] = x, z, r
    return _drift["x"], _drift["z"], _drift["r"]


def _drift_queries(x, z, busy):
    """The busy waves' 64 queries sit at x: every 16-ref tile of every stream holds a new record.  The other waves'
    queries sit at z: their nearest ref of every stream is its first one, the copy of z in the first tile, and no ref of
    the line comes within 5 of it — far outside the bound B8 and the margin, which are below 1 at these magnitudes — so
    they flag once per stream and run on to the next barrier, where they wait for the busy wave."""
    q = np.repeat(z[None, :], M, axis=0)
    for w in busy:
        q[64 * w:64 * w + 64] = x
    return q


@pytest.mark.parametrize("busy", [(0,), (7,), (3, 7)], ids=["wave0", "wave7", "wave3_and_partner7"])
def test_cadence_maximum_drift(pkg, orc, busy):
    """One wave (or the two waves of one SIMD) refines every tile of every stream while the other waves refine next to
    nothing: the largest distance the barriers allow between the waves of a workgroup, over three turns of the ring."""
    x, z, r = _drift_refs(pkg)
    q = _drift_queries(x, z, busy)
    group = np.concatenate([np.arange(64 * w, 64 * w + 64, 9) for w in busy])
    idx, _ = _check(pkg, orc, q, r, group=group, sample=32)
    quiet = np.ones(M, bool)
    for w in busy:
        quiet[64 * w:64 * w + 64] = False
        assert (idx[64 * w:64 * w + 64] == r.shape[0] - 1).all()     # the line's last ref
    assert (idx[quiet] == idx[quiet][0]).all() and idx[quiet][0] % (DRIFT_SLOTS * SLOT) == 0   # a stream's first ref


def test_cadence_drift_is_repeatable(pkg):
    """The drift case three times on one index: bit-equal keys, the same exact-scan and multi-candidate counts."""
    x, z, r = _drift_refs(pkg)
    q = _drift_queries(x, z, (3, 7))
    qd = torch.from_numpy(q).cuda()
    ix = pkg.Index(torch.from_numpy(r).cuda(), path="mfma_perref", filter_i8pre="force")
    runs = [_keys(pkg, ix, qd, True) for _ in range(3)]
    ix.close()
    for keys, st in runs[1:]:
        assert torch.equal(keys, runs[0][0])
        assert st["ambiguous"] == runs[0][1]["ambiguous"] and st["multi_candidate"] == runs[0][1]["multi_candidate"], (st, runs[0][1])


# ---- neighbours at group edges ------------------------------------------------------------------------------------------
def test_cadence_neighbours_at_group_edges(pkg, orc):
    """Streams of 3 G + 5 slots.  For g = 1, 2 a query's true nearest ref sits in the last tile of slot g G - 1, in the first
    tile of slot g G (the interval that opens with the barrier), and in slot g G + G (first read, for the prefetch and the
    seeds, from the group before — across the barrier); six queries on six different waves, each with a near tie one ulp
    farther in another stream."""
    slots = 3 * G + 5
    n, p = _n_for(pkg, slots)
    q, r = _uniform(pkg, M, n, K, 3301)
    split, tie_split = 7, p["splits"] - 3
    want = {}
    places = [(g * G - 1, 48 + 5) for g in (1, 2)] + [(g * G, 2) for g in (1, 2)] + [(g * G + G, 16 + 9) for g in (1, 2)]
    for w, (slot, row) in enumerate(places):
        i = 64 * w + 7 * w + 1
        j = (split * slots + slot) * SLOT + row
        jt = (tie_split * slots + slot) * SLOT + row
        assert j < n and jt < n and j != jt
        c = (3 * w) % K
        r[j] = q[i]
        r[j, c] = _ulp_up(r[j, c])
        r[jt] = q[i]
        r[jt, c] = _ulp_up(_ulp_up(r[jt, c]))
        want[i] = j
    idx, _ = _check(pkg, orc, q, r, group=list(want), sample=64)
    assert all(idx[i] == j for i, j in want.items()), [(i, idx[i], j) for i, j in want.items()]
