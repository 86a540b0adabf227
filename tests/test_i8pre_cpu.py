"""CPU tests of the int8 pre-pass's arithmetic ("int8 pre-pass"): K2's quantisation emulated exactly in
numpy, the exported bound B8 (nns_i8pre_bound), the integer threshold the kernel derives in `tighten`, and the selection
rule on host-computed inputs.  The kernel's ISA: no scratch, 32 int8 MFMAs per slot on the hot path."""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_split_filter_cpu import _split  # noqa: E402

KT = 128
F = np.float32


def _quantise(v, cmax):
    """K2's fp32 arithmetic: t = fl(v * fl(127 / cmax)), r8 = clamp(rint(t), +-127), e = fl(t - r8)."""
    inv = F(F(127.0) / F(cmax))
    t = (v.astype(F) * inv).astype(F)
    r8 = np.clip(np.rint(t), -127, 127).astype(F)
    return r8.astype(np.int64), (t - r8).astype(F)


def _cmax(y):
    """mean_kernel's word: the largest centred |coordinate| times fl(1 + 2^-22), in fp32."""
    return F(F(np.abs(y).max()) * F(1.0 + 2.0 ** -22))


def _scale(y):
    return F(_cmax(y) / F(127.0))


def _families(rng):
    """(name, centred queries x' [16][128], centred refs y' [64][128])"""
    u = lambda *sh: (rng.random(sh, dtype=F) - F(0.5))  # noqa: E731
    y = u(64, KT)
    s = _scale(y)
    yield "uniform", u(16, KT), y
    # rint midpoints: t = n + 1/2 exactly, the largest quantisation error in every coordinate
    ym = ((rng.integers(-100, 100, (64, KT)) + 0.5) * s).astype(F)
    ym[0, 0] = F(126.9) * s
    yield "midpoints", ((rng.integers(-100, 100, (16, KT)) + 0.5) * _scale(ym)).astype(F), ym
    yield "clipped queries", (u(16, KT) * F(3.0)).astype(F), y
    yc = y.copy()
    yield "cancellation", (y[:16] + u(16, KT) * F(1e-3)).astype(F), yc
    yd = (u(64, KT) * F(1e-3)).astype(F)
    yd[:, 5] = u(64) * F(2.0)
    yield "one dominant dimension", (u(16, KT) * F(1e-3)).astype(F), yd
    # all three cross terms aligned: refs just below a midpoint in every coordinate (r8 = 101, e_y = +1/2), queries
    # likewise (q8 = 99, e_x = +1/2): q8.e_y, e_x.r8 and e_x.e_y are all positive and every
    # Cauchy-Schwarz step of the bound is an equality up to the one ref coordinate that fixes the scale
    s0 = F(1.0 / 127.0)
    ya = np.full((64, KT), F(101.5) * s0, F)
    ya[0, 0] = F(127.0) * s0
    yield "aligned midpoints", np.full((16, KT), F(99.5) * s0, F), ya
    yz = y.copy()
    yz[::4] = 0
    xz = u(16, KT)
    xz[::2] = 0
    yield "all-zero rows", xz, yz


def _three_product(x, y):
    xh, xl = _split(x)
    vh, vl = _split((F(-2.0) * y).astype(F))
    d = lambda t: t.astype(np.float64)  # noqa: E731
    return (d(y) ** 2).sum(1)[None, :] + d(xh) @ d(vh).T + d(xh) @ d(vl).T + d(xl) @ d(vh).T   # [query][ref]


def _bounds(pkg, x, y):
    s = _scale(y)
    r8, ey = _quantise(y, _cmax(y))
    q8, ex = _quantise(x, _cmax(y))
    r8max2 = F((r8 ** 2).sum(1).max())
    eymax2 = F((ey.astype(np.float64) ** 2).sum(1).max() * (1 + 2.0 ** -20))
    y2max = F((y.astype(np.float64) ** 2).sum(1).max())
    b8 = np.empty(x.shape[0])
    b = np.empty(x.shape[0])
    for i in range(x.shape[0]):
        x2 = F((x[i].astype(np.float64) ** 2).sum())
        c0 = pkg.tau_consts(KT, float(x2), float(y2max), 3)[0]
        ex2 = F((ex[i].astype(np.float64) ** 2).sum() * (1 + 2.0 ** -20))
        b8[i] = pkg.i8pre_bound(float(s), float(ex2), float((q8[i] ** 2).sum()), float(r8max2), float(eymax2), c0)
        b[i] = pkg.split_lazy_bound(KT, float(x2), float(y2max))
    seeds = np.floor((y.astype(np.float64) ** 2).sum(1) / (2.0 * float(s) ** 2)).astype(np.int64)
    acc = seeds[None, :] - q8 @ r8.T          # what a lane's accumulator holds: N_j - q8.r8, exact integers
    return float(s), acc, b8, b


def test_integer_accumulator_is_within_the_bound_and_the_threshold_excludes_nothing(pkg):
    rng = np.random.default_rng(811)
    tightest = 0.0
    for name, x, y in _families(rng):
        s, acc, b8, _ = _bounds(pkg, x, y)
        s3 = _three_product(x, y)
        unit = 2.0 * s * s
        # the accumulator, in score units, lies at most B8 above the three-product score, for every pair
        gap = acc * unit - s3
        assert (gap <= b8[:, None]).all(), (name, float((gap / b8[:, None]).max()))
        tightest = max(tightest, float((gap / b8[:, None]).max()))
        # the kernel's integer threshold (tighten, fp32): no pair with a three-product score <= thr is excluded
        inv = F(1.0) / (F(2.0) * F(s) * F(s))
        for thr in (s3.min(1), np.median(s3, 1), s3.max(1), s3.min(1) + 8e-3):
            w = ((thr.astype(F) + b8.astype(F)).astype(F) * inv).astype(F)
            wu = (w + np.abs(w) * F(2.0 ** -20) + F(1.0)).astype(F)
            thrw8 = np.clip(np.floor(wu), -(1 << 29), 1 << 29).astype(np.int64)
            inside = s3 <= thr.astype(F).astype(np.float64)[:, None]
            assert (acc[inside] <= np.broadcast_to(thrw8[:, None], acc.shape)[inside]).all(), name
        print(f"i8pre {name}: max (2 s^2 A - s3) / B8 = {float((gap / b8[:, None]).max()):.3f}")
    # not slack by construction: on the aligned family every inequality of the derivation is tight, and what remains — the
    # floor of the seed, the two integer units, c0 and the 2^-10 factor — is far below half the bound at these magnitudes
    assert tightest >= 0.5, tightest


def test_selection_rule_on_host_computed_inputs(pkg):
    """Uniform clouds pass; a ref cloud with one coordinate 1000 x the rest declines; m / 64 out-of-range queries still pass."""
    rng = np.random.default_rng(812)
    m, n = 512, 1024

    def odd_count(q, r):
        c = r.astype(np.float64).mean(0).astype(F)
        x, y = (q - c).astype(F), (r - c).astype(F)
        _, _, b8, b = _bounds(pkg, x, y)
        return int((b8 > F(1.5) * b.astype(F)).sum())

    r = rng.random((n, KT), dtype=F)
    q = rng.random((m, KT), dtype=F)
    assert odd_count(q, r) * 64 <= m
    ro = r.copy()
    ro[:, 7] *= F(1000.0)
    assert odd_count(q, ro) * 64 > m
    qc = q.copy()
    qc[:: 64][: m // 64] *= F(3.0)
    cnt = odd_count(qc, r)
    assert cnt * 64 <= m, cnt


def test_i8pre_kernel_isa_no_scratch_and_32_mfma_hot_path():
    """Through tools/isa_report.py (its line for the kernel and the listing it names), then the listing's slot loop."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import check_mfma_hazards as chk
    rep = subprocess.run([sys.executable, os.path.join(root, "tools", "isa_report.py")], check=True, stdout=subprocess.PIPE,
                         text=True).stdout.splitlines()
    (meta,) = [l for l in rep if "OpI8Pre" in l and " scratch " in l]   # (the report abbreviates the mangled name)
    f = meta.split()
    g = lambda k: int(f[f.index(k) + 1])  # noqa: E731
    assert g("scratch") == 0 and g("spill") == 0 and g("vgpr") <= 256, meta
    text = open(rep[-1].strip()).read()
    kern = chk.split_kernels(text.splitlines(), which=r"filter_i8pre_kernel", end=".Lfunc_end")
    (lines,) = kern.values()
    body = [l.split(";")[0].strip() for _, l in lines]
    labels = {l[:-1]: i for i, l in enumerate(body) if re.fullmatch(r"\.LBB\d+_\d+:", l)}
    # the slot loop's interval: from its barrier (the last one of the kernel) along the fall-through path, cold branches
    # not taken, to the loop's back-edge — the last conditional branch to a label at or before the barrier
    bar = max(j for j, l in enumerate(body) if l.startswith("s_barrier"))
    i, walk = bar, []
    while i not in walk and not body[i].startswith("s_endpgm"):
        walk.append(i)
        i = labels[body[i].split()[1]] if body[i].startswith("s_branch") else i + 1
    back = [j for j in walk if body[j].startswith("s_cbranch") and labels.get(body[j].split()[-1], len(body)) <= bar]
    assert back, "no back-edge on the fall-through path"
    back_edge = back[-1]
    path = [body[j] for j in walk if j <= back_edge]
    assert sum(l.startswith("v_mfma_i32_16x16x64_i8") for l in path) == 32
    assert not any(l.startswith("v_mfma_f32") for l in path)        # the refinement's bf16 MFMAs are off the hot path
    assert sum(l.startswith("ds_read_b128") for l in path) <= 12    # 8 fragments + the seeds
    assert not any(l.startswith(("scratch_", "buffer_")) for l in path)
    # the cold branch is laid out behind the loop: every refinement MFMA sits after the loop's back-edge, none between the
    # loop's barrier and it
    first_cold = min(j for j, l in enumerate(body) if l.startswith("v_mfma_f32_16x16x32_bf16"))
    assert first_cold > back_edge, (first_cold, back_edge)
    nref = sum(l.startswith("v_mfma_f32_16x16x32_bf16") for l in body)   # 12 per refined (ref tile, state), laid out cold
    assert nref >= 12 * 8 and nref % 12 == 0, nref
