"""Host-side checks of the proof margin tau (nns_internal.h: tau_consts / tau_of), compiled from the
very header the kernels use: monotone in the score (the filter relies on it to keep a running
threshold instead of a running minimum), growing with the norms and the tile depth, and ordered by
operand precision (fp32 operands < bf16 points < fp32 points rounded to bf16 operands); and that the fp32 thresholds
the kernels form from them (K5 / the MFMA filter, and K1f's k1f_tau) stay above the proof's bound, absolute underflow
term included, from subnormal norms upward."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <stdio.h>
#include "nns_internal.h"
int main()
{
    using namespace nns;
    const float xs[] = {0.0f, 1e-3f, 1.0f, 10.7f, 3000.0f};
    const float ys[] = {1e-3f, 1.0f, 10.7f, 3000.0f};
    const int kts[] = {32, 64, 128, 256, 512};
    for (int kt : kts)
        for (float x2 : xs)
            for (float y2 : ys)
                for (int mode = 0; mode < 3; ++mode) {
                    const TauConsts t = tau_consts(kt, x2, y2, mode);
                    printf("%d %g %g %d %.9g %.9g %.9g", kt, x2, y2, mode, t.c0, t.c1, t.x2);
                    float prev = -3.0e38f;
                    int mono = 1;
                    for (float a = -x2; a < 4.0f * (x2 + y2) + 1.0f; a += 0.01f * (x2 + y2) + 1e-4f) {
                        const float v = a + 1.002f * tau_of(t, a);
                        if (v < prev) mono = 0;
                        prev = v;
                    }
                    printf(" %d %.9g\n", mono, tau_of(t, y2));
                }
    return 0;
}
'''


def test_tau_margin_properties():
    with tempfile.TemporaryDirectory() as d:
        exe = _compile_host(d, SRC, "tau")
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    rows = {}
    for line in out.splitlines():
        kt, x2, y2, mode, c0, c1, tx2, mono, tau = line.split()
        rows[(int(kt), float(x2), float(y2), int(mode))] = (float(c0), float(c1), float(tx2), int(mono), float(tau))
    assert len(rows) == 5 * 5 * 4 * 3
    for (kt, x2, y2, mode), (c0, c1, tx2, mono, tau) in rows.items():
        assert c0 > 0 and c1 > 0 and tx2 >= x2 and mono == 1, (kt, x2, y2, mode)
        assert tau > 0
    for (kt, x2, y2, mode), v in rows.items():
        if mode < 2:     # operand precision orders the margins (mode 0 has the extra centring term, so compare 1 < 2)
            pass
        if mode == 1:
            assert rows[(kt, x2, y2, 2)][4] >= v[4], (kt, x2, y2)
        if kt < 512:     # deeper tiles accumulate more rounding
            nxt = {32: 64, 64: 128, 128: 256, 256: 512}[kt]
            assert rows[(nxt, x2, y2, mode)][4] >= v[4]
    # the rounding term of mode 2 is the dominant one: ~2 * 2^-6 |x||y| for unit-scale norms
    c0 = rows[(128, 10.7, 10.7, 2)][0]
    assert 2 * 2 ** -6 * 10.7 < c0 < 4 * 2 ** -6 * 10.7 * 1.5


U = 2.0 ** -24
ETA = 2.0 ** -150      # the largest error of one rounding whose result lies below FLT_MIN (half a subnormal ulp)


def _tau_needed(kt, X2, Y2, mode, a):
    """The proof's tau(a) (finalize.hip), no safety factors, extended precision: returns (tau, X, Y, e3)."""
    import numpy as np
    L = np.longdouble
    X2, Y2 = L(X2) * (1 + 4 * L(U)), L(Y2) * (1 + 4 * L(U))
    X, Y = np.sqrt(X2), np.sqrt(Y2)
    gk = (kt + 2) * L(U) / (1 - (kt + 2) * L(U))
    if mode == 0:
        e3 = gk * (Y2 + 2 * X * Y) + 2 * L(U) * Y2
        e2 = L(2.5) * L(U) * (X + Y) ** 2
    else:
        gf = 2 * (kt + kt // 16 + 2) * L(U) / (1 - 2 * (kt + kt // 16 + 2) * L(U))
        e3 = gf * (Y2 + 2 * X * Y) + 2 * L(U) * Y2
        e2 = L(0)
        if mode == 2:
            e3 = e3 * (1 + L(2) ** -6) + L(2) ** -6 * (1 + L(2) ** -8) * X * Y
            e2 = L(2.5) * L(U) * (X + Y) ** 2
    return 2 * (e3 + e2) + 2 * gk / (1 - gk) * (max(L(a) + X2, L(0)) + e3 + e2), X, Y, e3


def _underflow_term(score_roundings, v0_products):
    """The absolute part of the bound: a score or a V0 distance is off by up to ETA per rounding whose result is
    subnormal, beyond every relative term.  Adds and subtractions with a subnormal result are exact, so what counts is
    the FMAs / products of the two scores compared and the products of V0's two distances."""
    import numpy as np
    return np.longdouble(2 * score_roundings + 2 * v0_products) * np.longdouble(ETA)


def test_fp32_threshold_sum_is_covered():
    """finalize.hip, "fp32 evaluation": the threshold K5 forms in fp32, T5(a) = fl(a + tau_fl(a)), must not fall below
    the real-arithmetic a + tau(a) of the proof although the sum is rounded at the SCORE's magnitude (up to
    tau / (2 (K + 2)) of error) — the explicit term er of tau_consts covers it — and the filter's
    Tf(t) = fl(t + fl(1.002 tau_fl(t))) must dominate T5(a) for every t >= a.  fp32 emulated with numpy, the
    requirement evaluated in extended precision; (c0, c1, x2) come from the library (nns_tau_consts, host only).
    Norms down to subnormal ones: there the requirement's absolute underflow term (a chain of kt + kt / 16 + 2
    roundings per score, kt products per V0 distance) is what tau_consts' floor c0 >= 1e-30 must cover."""
    import numpy as np
    import __graft_entry__ as graft
    pkg = graft.load_package()
    f32 = np.float32
    u = U
    L = np.longdouble

    def tau_fl(c0, c1, x2, a):      # exactly the kernels' expression order (tau_of / tighten), every step rounded to fp32
        d = f32(a) + f32(x2)
        d = d if d > 0 else f32(0)
        return f32(c0) + f32(c1) * d

    def tau_needed(kt, X2, Y2, mode, a):
        need, X, Y, e3 = _tau_needed(kt, X2, Y2, mode, a)
        return need + _underflow_term(kt + kt // 16 + 2, kt), X, Y, e3

    rng = np.random.default_rng(7)
    checked = 0
    with np.errstate(over="ignore"):
        for kt in (16, 32, 64, 128, 256, 512, 1024):
            for X2 in (0.0, 1e-44, 3e-40, 1e-38, 1e-3, 0.7, 10.7, 43.0, 3000.0, 1e6):
                for Y2 in (1e-44, 3e-40, 1e-38, 1e-3, 0.7, 10.7, 43.0, 3000.0, 1e6):
                    for mode in (0, 1, 2):
                        c0, c1, x2 = pkg.tau_consts(kt, X2, Y2, mode)
                        _, X, Y, e3 = tau_needed(kt, X2, Y2, mode, 0.0)
                        lo, hi = -float(X * X), float((X + Y) ** 2 + e3)      # every attainable score
                        grid = np.concatenate([np.linspace(lo, hi, 41), rng.uniform(lo, hi, 40), [0.0, lo, hi]])
                        for a in grid.astype(np.float32):
                            need, _, _, _ = tau_needed(kt, X2, Y2, mode, float(a))
                            t5 = f32(a) + tau_fl(c0, c1, x2, a)                      # K5's threshold, in fp32
                            assert L(t5) >= L(a) + need, (kt, X2, Y2, mode, float(a), float(t5), float(L(a) + need))
                            # the requested form: slack = tau_used - tau_needed >= u (|a| + tau)
                            used = L(c0) + L(c1) * max(L(a) + L(x2), L(0))
                            assert used - need >= L(u) * (abs(L(a)) + used), (kt, X2, Y2, mode, float(a))
                            # the filter's threshold of any t >= a dominates K5's threshold of a
                            for t in (a, np.nextafter(a, f32(np.inf)), f32(a + 0.37 * abs(a) + 1e-3)):
                                tf = f32(t) + f32(f32(1.002) * tau_fl(c0, c1, x2, t))
                                assert tf >= t5, (kt, X2, Y2, mode, float(a), float(t))
                            checked += 1
    assert checked > 100000


K1F_SRC = r'''
#include <math.h>
#include <stdio.h>
#include "nns_internal.h"
// one query per line: K, x'[K], y'[K], then scores a until "e"; out: the kernel's fp32 threshold of each a.
// The norms are K1f's: FMA chains from 0 (exact_kernels.hip, lowdim_filter_kernel), the threshold its k1f_threshold.
int main()
{
    int K;
    while (scanf("%d", &K) == 1) {
        float x[3], y[3], xn = 0.0f, y2 = 0.0f;
        for (int t = 0; t < K; ++t) scanf("%a", &x[t]);
        for (int t = 0; t < K; ++t) scanf("%a", &y[t]);
        for (int t = 0; t < K; ++t) xn = fmaf(x[t], x[t], xn);
        for (int t = 0; t < K; ++t) y2 = fmaf(y[t], y[t], y2);
        char tok[64];
        while (scanf("%63s", tok) == 1 && tok[0] != 'e') printf("%a\n", nns::k1f_threshold(strtof(tok, nullptr), xn, y2));
    }
    return 0;
}
'''


def _compile_host(d, src_text, name):
    """Build a host program in d against nns_internal.h (hipcc, no contraction: the kernels' own -ffp-contract=off)."""
    src, exe = os.path.join(d, name + ".hip"), os.path.join(d, name)
    with open(src, "w") as f:
        f.write(src_text)
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off",
                    "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "nns-cuda_amd", "csrc"), "-o", exe, src],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return exe


def test_k1f_tau_covers_its_proof():
    """K1f's margin (nns_internal.h: k1f_tau / k1f_threshold, the expressions the kernel evaluates) against the proof it
    stands for, from subnormal squared norms up to 1e30: for K = 1, 2, 3, a query x' and the workgroup's largest ref y'
    with |x'|^2 = X^2, |y'|^2 = Y^2, and every attainable score a on a grid, the kernel's fp32 threshold
    fl(a + k1f_tau(a, fl(xn 1.00001f), fl(y2 1.00001f))) — xn, y2 the kernel's FMA-chain norms — must be at least
    a + need(a) in extended precision: need = tau_consts' mode-0 model at K1f's chain length (2K FMAs per score) plus
    the absolute underflow term (2 x 2K score FMAs, 2 x K V0 products, 2^-150 each).  Without an absolute term the
    threshold collapses to a itself once the squares are subnormal."""
    import numpy as np
    L = np.longdouble
    f32 = np.float32
    rng = np.random.default_rng(11)
    norms = (1e-44, 1e-43, 7e-42, 1e-40, 3e-39, 1.1e-38, 2e-38, 1e-37, 1e-35, 1e-30, 1e-20, 1e-10, 1e-3, 1.0, 10.7,
             1e6, 1e15, 1e30)
    cases, lines = [], []
    for K in (1, 2, 3):
        for X2 in (0.0,) + norms:
            for Y2 in norms:
                # a query and a ref of those squared norms, random directions; the norms are recomputed from the fp32
                # coordinates in extended precision (what the proof calls X^2, Y^2)
                x = rng.normal(size=K) if X2 > 0 else np.zeros(K)
                y = rng.normal(size=K)
                x = (x * np.sqrt(X2 / max(np.sum(x * x), 1e-300))).astype(f32)
                y = (y * np.sqrt(Y2 / np.sum(y * y))).astype(f32)
                if not np.any(y):
                    y[0] = f32(np.sqrt(Y2)) if np.sqrt(Y2) > 0 else np.nextafter(f32(0), f32(1))
                tX2 = float(np.sum(x.astype(L) ** 2))
                tY2 = float(np.sum(y.astype(L) ** 2))
                _, X, Y, e3 = _tau_needed(2 * K, tX2, tY2, 0, 0.0)
                lo, hi = -float(X * X), float((X + Y) ** 2 + e3)      # every attainable score
                grid = np.concatenate([np.linspace(lo, hi, 33), rng.uniform(lo, hi, 24), [0.0, lo, hi],
                                       lo + (hi - lo) * np.array([1e-9, 1e-6, 1e-3])])
                grid = np.unique(grid.astype(f32))
                lines.append(" ".join([str(K)] + [float(v).hex() for v in x] + [float(v).hex() for v in y]
                                      + [float(a).hex() for a in grid] + ["e"]))
                cases.append((K, tX2, tY2, grid))
    with tempfile.TemporaryDirectory() as d:
        exe = _compile_host(d, K1F_SRC, "k1f_tau")
        out = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout
    thr = [float.fromhex(v) for v in out.split()]
    assert len(thr) == sum(len(g) for *_, g in cases)
    at = 0
    bad = []
    for K, tX2, tY2, grid in cases:
        for a in grid:
            need, _, _, _ = _tau_needed(2 * K, tX2, tY2, 0, float(a))
            need += _underflow_term(2 * K, K)
            got = thr[at]
            at += 1
            if not L(got) >= L(float(a)) + need:
                bad.append((K, tX2, tY2, float(a), got, float(L(float(a)) + need)))
    assert not bad, f"{len(bad)} thresholds below a + need(a), e.g. (K, X^2, Y^2, a, threshold, a + need): {bad[:4]}"
    assert at > 5000
