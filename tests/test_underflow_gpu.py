"""GPU parity at underflow scale: every search kernel on data whose squared coordinates or distances are subnormal
(or round to 0), against the V0 oracle — indices exact, distances bit for bit.  Each case is pinned to the kernel it
claims to test by the planner (nns_plan_exact / _filter / _topk / _range).

Why: the filters' margins are relative bounds plus an absolute floor (tau_consts: 1e-30; K1f's k1f_tau: 2^-144,
nns_internal.h); below FLT_MIN every rounding is off by up to 2^-150 however small its operands, and a flush-to-zero
anywhere (a build flag, an intrinsic) would change V0's bits.  Families:
  sub20 / sub21 / sub22   uniform clouds scaled by 1e-20 / 1e-21 / 1e-22: subnormal squares
  flt_min                 scaled by 1e-19: squares on both sides of FLT_MIN
  zero                    scaled by 1e-23: every square rounds to 0, all distances tie at 0 (the lowest index wins)
  offset18 / offset17     1e-18 + 1e-21 U, 1e-17 + 3e-21 U: normal coordinates, subnormal differences
  mixed                   unit-scale points with some subnormal coordinates
  ties                    a 1e-21 cloud and planted queries outside it, each with a winner and three rivals at
                          subnormal squared distances 4 - 90 ulps apart, the winner in a later 16-ref chunk than its
                          rivals (K1f re-ranks two chunks per query: the margin decides whether that is enough);
                          _cloud checks that every planted winner is V0's answer
At k <= 3 the refs of K1f's shapes are dense enough that the fixed scales above give exact zero-distance winners
only, so test_k1f_underflow adds clouds scaled to the ref density (K1F_SCALES): there V0's winners have NONZERO
subnormal distances, which the test asserts from the oracle's answers.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_parity import _bits, _check, _check_bf16  # noqa: E402
from test_range_cpu import range_oracle, v0_all  # noqa: E402
from test_range_gpu import _assert_same as _assert_same_range, _index_range  # noqa: E402
from test_topk_edges_gpu import _as_searched, _to_dev, _whole as _whole_topk  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32 = np.float32
NNS_FILTER_BF16 = 128
FAMILIES = ("sub20", "sub21", "sub22", "flt_min", "zero", "offset18", "offset17", "mixed", "ties")


def _cloud(family, seed, m, n, k):
    """(q, r) fp32 of one data family (module docstring)."""
    rng = np.random.default_rng(seed)
    q = rng.random((m, k), dtype=F32)
    r = rng.random((n, k), dtype=F32)
    scale = {"sub20": 1e-20, "sub21": 1e-21, "sub22": 1e-22, "flt_min": 1e-19, "zero": 1e-23, "ties": 1e-21}
    if family in scale:
        q, r = q * F32(scale[family]), r * F32(scale[family])
    elif family == "offset18":
        q, r = F32(1e-18) + q * F32(1e-21), F32(1e-18) + r * F32(1e-21)
    elif family == "offset17":
        q, r = F32(1e-17) + q * F32(3e-21), F32(1e-17) + r * F32(3e-21)
    elif family == "mixed":
        for a in (q, r):
            hit = rng.random(a.shape) < 0.1
            a[hit] = rng.random(int(hit.sum()), dtype=F32) * F32(1e-38)       # subnormal coordinates
    elif family.startswith("denseoff"):  # denseoff<scale>: that cloud moved to 64 x scale (normal coordinates)
        s = F32(float(family[8:]))
        q, r = F32(64) * s + q * s, F32(64) * s + r * s
    elif family.startswith("dense"):     # dense<scale>: a cloud of that scale (K1F_SCALES)
        s = F32(float(family[5:]))
        q, r = q * s, r * s
    if family == "ties":
        _plant_ties(rng, q, r, k)
    assert np.isfinite(q).all() and np.isfinite(r).all()
    if family in ("sub20", "sub21", "sub22"):
        d = (q[:8, None, :] - r[None, :512, :]) ** 2
        assert ((d > 0) & (d < np.finfo(F32).tiny)).mean() > 0.3               # most squares are subnormal (1e-22: or 0)
    return q, r


def _plant_ties(rng, q, r, k):
    """The ties family: planted queries 10, 20, ... cloud widths outside the 1e-21 cloud (in coordinate 0), each with four
    planted refs q + offset e_t in four distinct 16-ref chunks: rivals in the lower chunks at offsets 1e-21 (1 + U(0.003,
    0.06)), the winner at 1e-21 in the highest one.  Squared distances are about 714 subnormal ulps, the rivals 4 - 90
    ulps above the winner: some within K1f's floor (ambiguous queries), some beyond it (the two-chunk re-rank)."""
    m, n = q.shape[0], r.shape[0]
    planted = min(m, 64, n // 64)
    chunks = rng.choice(n // 16, size=4 * planted, replace=False).reshape(planted, 4)
    chunks.sort(axis=1)
    win = np.empty(planted, np.int64)
    for i in range(planted):
        q[i, 0] += F32(1e-20 * (1 + i))                                       # planted queries 1e-20 apart
        offs = np.concatenate([1.0 + rng.uniform(0.003, 0.06, 3), [1.0]])     # rivals first, the winner last
        for c in range(4):
            j = 16 * int(chunks[i, c]) + int(rng.integers(0, 16))
            r[j] = q[i]
            r[j, int(rng.integers(0, k))] += F32(offs[c] * 1e-21)
        win[i] = j
    # every planted winner is V0's answer (first minimum = V0's lowest-index rule), at a nonzero subnormal distance
    d = v0_all(q[:planted], r)
    assert np.array_equal(np.argmin(d, axis=1), win)
    best = d[np.arange(planted), win]
    assert ((best > 0) & (best < np.finfo(F32).tiny)).all()


def _index_check(pkg, orc, q, r, **kw):
    """Index (device-resident refs) search against the oracle."""
    want_idx, want_dist = orc.v0_search(q, r, threads=8)
    ix = pkg.Index(torch.from_numpy(r).to(DEV), **kw)
    idx, dist = ix.search(torch.from_numpy(q).to(DEV), return_distances=True)
    torch.cuda.synchronize()
    ix.close()
    assert np.array_equal(idx.cpu().numpy(), want_idx), f"Index {kw}: index mismatches"
    assert np.array_equal(_bits(dist.cpu().numpy()), _bits(want_dist)), f"Index {kw}: distance bits differ"


# ---- K1f: the vector-ALU filter + re-rank of k <= 3 from 2^27 pairs ------------------------------------------------
# Cloud scales at which K1f's 65549 refs leave V0's winners at NONZERO subnormal squared distances (the first three)
# or on both sides of FLT_MIN (the last): the nearest-ref spacing is about scale x n^(-1/k).
K1F_SCALES = {1: (1e-17, 1e-16, 1e-15, 1e-14), 2: (1e-19, 1e-18, 1e-17, 1e-16), 3: (1e-20, 1e-19, 1e-18, 1e-17)}


@pytest.mark.timeout(900)
@pytest.mark.parametrize("k", [1, 2, 3])
def test_k1f_underflow(pkg, orc, k):
    m, n = 4096 + 37, 65536 + 13        # ragged; >= 2^27 pairs per shard with one and with two shards
    assert pkg.plan_exact(k, m, n)["kernel"] == "k1f"
    assert pkg.plan_exact(k, m, (n + 1) // 2)["kernel"] == "k1f"
    tiny = np.finfo(F32).tiny
    dense = [f"dense{s:g}" for s in K1F_SCALES[k]] + [f"denseoff{K1F_SCALES[k][1]:g}"]
    for i, fam in enumerate(FAMILIES + tuple(dense)):
        q, r = _cloud(fam, 1000 * k + i, m, n, k)
        if fam.startswith("dense"):
            with np.errstate(all="ignore"):
                _, d = orc.v0_search(q, r, threads=8)
            sub, normal = ((d > 0) & (d < tiny)).mean(), (d >= tiny).mean()
            if fam == dense[3]:
                assert sub > 0.1 and normal > 0.1, (fam, sub, normal)     # winners on both sides of FLT_MIN
            else:
                assert sub > 0.6, (fam, sub)                             # winners at nonzero subnormal distances
        with np.errstate(all="ignore"):
            _check(pkg, orc, q, r, paths=("auto", "exact"), shards=(1, 2))
            if fam in ("sub21", "ties", "offset18", dense[1]):
                _index_check(pkg, orc, q, r, path="exact")


# ---- K1a / K1c / K1b: the exact kernels ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 4, 8, 16, 32])
def test_exact_kernels_underflow(pkg, orc, k):
    for m, n, kernel in ((100, 5000, "k1a" if k != 32 else "k1b"), (1, 70001, "k1c"), (3, 4097, "k1c"),
                         (20, 3000, "k1b")):
        assert pkg.plan_exact(k, m, n)["kernel"] == kernel, (k, m, n)
        assert pkg.plan_exact(k, m, (n + 1) // 2)["kernel"] == kernel, (k, m, n)     # each of the two shards
        for fam in ("sub20", "sub22", "flt_min", "zero", "offset18", "mixed", "ties"):
            q, r = _cloud(fam, 7 * k + m + FAMILIES.index(fam), m, n, k)
            _check(pkg, orc, q, r, paths=("exact",), shards=(1, 2))


def test_k1b_fallback_underflow(pkg, orc):
    """Refs 4 bytes off a 16-byte boundary are not K1c's: the lane-per-ref K1b takes over (as in
    test_k1c_streaming_kernel_few_queries)."""
    k, n = 16, 5000
    for fam in ("sub21", "flt_min", "zero", "offset17"):
        q, r = _cloud(fam, 70 + FAMILIES.index(fam), 2, n, k)
        flat = torch.zeros(n * k + 1, dtype=torch.float32, device=DEV)
        flat[1:].copy_(torch.from_numpy(r.ravel()))
        r_off = flat[1:].view(n, k)
        assert r_off.data_ptr() % 16 == 4
        assert pkg.plan_exact(k, 2, n, refs_aligned=False)["kernel"] == "k1b"
        want_idx, want_dist = orc.v0_search(q, r, threads=8)
        ix = pkg.Index(r_off, path="exact")
        idx, dist = ix.search(torch.from_numpy(q).to(DEV), return_distances=True)
        torch.cuda.synchronize()
        ix.close()
        assert np.array_equal(idx.cpu().numpy(), want_idx), fam
        assert np.array_equal(_bits(dist.cpu().numpy()), _bits(want_dist)), fam


# ---- the MFMA filter (K3) + K5 re-rank, bf16 points (K4), the opt-in bf16 filter on fp32 points ---------------------
@pytest.mark.parametrize("k,kt", [(16, 16), (64, 64), (128, 128), (200, 256)])
def test_mfma_filter_underflow(pkg, orc, k, kt):
    m, n = 130, 3000
    assert pkg.plan_filter(k, m, n)["kt"] == kt and pkg.plan_filter(k, m, (n + 1) // 2)["kt"] == kt
    for fam in ("sub20", "sub22", "flt_min", "zero", "offset18", "mixed", "ties"):
        q, r = _cloud(fam, 300 + k + FAMILIES.index(fam), m, n, k)
        _check(pkg, orc, q, r, paths=("mfma",), shards=(1, 2))      # both record forms (mfma, mfma_perref)


@pytest.mark.parametrize("k", [64, 256])
def test_bf16_points_underflow(pkg, orc, k):
    m, n = 130, 3000
    p = pkg.plan_filter(k, m, n, bf16=True)
    assert p["bf16"] == 1 and p["mixed"] == 0
    for fam in ("sub20", "sub22", "flt_min", "zero", "mixed", "bf16_subnormal"):
        if fam == "bf16_subnormal":          # every coordinate a bf16 subnormal (x 2^-133 .. 2^-127), or 0
            rng = np.random.default_rng(400 + k)
            q = rng.integers(0, 128, (m, k)).astype(F32) * F32(2.0 ** -133)
            r = rng.integers(0, 128, (n, k)).astype(F32) * F32(2.0 ** -133)
            assert np.array_equal(pkg.to_bf16_bits(r).astype(np.uint32) << 16, r.view(np.uint32))   # exact in bf16
        else:
            q, r = _cloud(fam, 400 + k + FAMILIES.index(fam), m, n, k)
        _check_bf16(pkg, orc, q, r, paths=("auto", "mfma", "exact"), shards=(1, 2))


def test_bf16_filter_on_fp32_points_underflow(pkg, orc):
    k, m, n = 64, 130, 3000
    assert pkg.plan_filter(k, m, n, flags=NNS_FILTER_BF16)["mixed"] == 1
    for fam in ("sub20", "sub22", "flt_min", "zero", "offset18", "mixed", "ties"):
        q, r = _cloud(fam, 500 + FAMILIES.index(fam), m, n, k)
        want_idx, want_dist = orc.v0_search(q, r, threads=8)
        for path in ("mfma", "mfma_perref"):
            for s in (1, 2):
                idx, dist = pkg.search(q, r, return_distances=True, shards=s, path=path, filter_bf16=True)
                assert np.array_equal(idx, want_idx), (fam, path, s)
                assert np.array_equal(_bits(dist), _bits(want_dist)), (fam, path, s)


# ---- top-K (K6) and range search (K7) -------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_topk_underflow(pkg, bf16):
    k, m, n, kn = 16, 40, 3000, 10
    assert pkg.plan_topk(k, m, n, kn, bf16=bf16)["queries_per_wg"] > 0
    for fam in ("sub21", "flt_min", "zero", "offset17", "mixed", "ties"):
        q, r = _cloud(fam, 600 + FAMILIES.index(fam), m, n, k)
        _whole_topk(pkg, q, r, kn, bf16)
        _whole_topk(pkg, q, r, kn, bf16, shards=2)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_range_subnormal_radius(pkg, bf16):
    """Count and fill with a subnormal radius2 taken from the distances themselves: one exactly at an attained
    distance (inclusive: that ref is in) and its nextafter below (it is out)."""
    k, m, n = 3, 50, 4000
    for fam in ("sub21", "sub22", "flt_min", "ties") + (() if bf16 else ("offset18",)):
        q, r = _cloud(fam, 700 + FAMILIES.index(fam), m, n, k)
        q, r = _as_searched(pkg, q, bf16), _as_searched(pkg, r, bf16)
        assert pkg.plan_range(k, m, n, bf16=bf16)["chunks"] >= 1
        d = v0_all(q, r)
        sub = np.unique(d[(d > 0) & (d < np.finfo(F32).tiny)])
        assert sub.size >= 3, fam
        at = F32(sub[sub.size // 3])
        radii = (at, np.nextafter(at, F32(0)), F32(sub[0]), F32(sub[-1]))
        wants = [range_oracle(q, r, x) for x in radii]
        assert wants[0][0][-1] > wants[1][0][-1]          # the radius at an attained distance admits more refs
        for x, want in zip(radii, wants):
            if bf16:
                got = pkg.search_range_bf16(pkg.to_bf16_bits(q), pkg.to_bf16_bits(r), float(x), return_distances=True)
            else:
                got = pkg.search_range(q, r, float(x), return_distances=True)
            _assert_same_range(got, want, f"whole {fam} bf16={bf16} r2={float(x)!r}")
        got = _index_range(pkg, _to_dev(pkg, r, bf16), _to_dev(pkg, q, bf16), float(at), path="exact")
        _assert_same_range(got, wants[0], f"split {fam} bf16={bf16}")
