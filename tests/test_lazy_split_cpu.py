"""CPU tests of the lazy schedule of the split-bf16 filter (OpLazySplitT): the exported bound B covers how far a pair's
three-product score can lie below its hi-hi partial score — the split emulated exactly in numpy, both sums taken in
the lazy order — and is the right size, not merely large; fl(thr + B) in fp32 never falls below the real thr + B_needed;
default plans report the lazy schedule exactly where the library enables it and move no other field; the flag
combinations that must be rejected are; and the lazy kernels' ISA is unrolled, hazard-free and spill-free."""
import importlib.util
import math
import os
import re

import numpy as np
import pytest

from test_filter_cases_cpu import FILTER_CASES
from test_split_filter_cpu import _families, _split

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
KTS = (16, 32, 64, 128, 256)      # every fp32 depth built
LAZY_KTS = (128,)                 # depths whose long streams run the lazy kernel (filter_mfma.hip, lazy_depth)


def _parts(x, v, flush):
    qh, ql = _split(x)
    rh, rl = _split(v)
    if flush:
        qh, ql, rh, rl = (np.where(np.abs(t) < 2.0 ** -126, np.float32(0), t) for t in (qh, ql, rh, rl))
    return qh, ql, rh, rl


def _lazy_sums_f32(seed, qh, ql, rh, rl):
    """(s_hh, s_3) of one pair with every add rounded to fp32, in the lazy order: the seed, the hi-hi products of all
    k-steps, then per 16-dim k-step rh x ql and rl x qh.  (bf16 x bf16 products are exact in fp32.)"""
    f32 = np.float32
    acc = f32(seed)
    with np.errstate(over="ignore", under="ignore"):
        for t in range(len(qh)):
            acc = f32(acc + f32(qh[t] * rh[t]))
        s_hh = acc
        for s in range(len(qh) // 16):
            for t in range(16 * s, 16 * s + 16):
                acc = f32(acc + f32(rh[t] * ql[t]))
            for t in range(16 * s, 16 * s + 16):
                acc = f32(acc + f32(rl[t] * qh[t]))
    return s_hh, acc


def _b_needed(kt, Y2, qh, ql, rh, rl):
    """s_hh - s_3 at its largest under the accumulation model: minus the exact cross sum, plus 2u per add over the
    2 kt products and 2 kt / 16 MFMA-level adds on partial sums of magnitude <= Y^2 + sum |products|, plus 2^-126 per
    product or add whose result is below 2^-126."""
    d = lambda t: t.astype(np.float64)   # noqa: E731
    cross = math.fsum(np.concatenate([d(qh) * d(rl), d(ql) * d(rh)]))
    sumprod = math.fsum(np.abs(np.concatenate([d(qh) * d(rh), d(qh) * d(rl), d(ql) * d(rh)])))
    nb = 2 * kt + 2 * (kt // 16)
    g = 2 * nb * U / (1 - 2 * nb * U)
    return -cross + g * (Y2 * (1 + 4 * U) + sumprod) + (2 * kt + nb) * 2.0 ** -126


def test_bound_covers_the_cross_products_in_the_lazy_order(pkg):
    f32 = np.float32
    L = np.longdouble
    rng = np.random.default_rng(777)
    checked = 0
    for kt in KTS:
        for name, x, v in _families(rng, kt):
            for flush in (False, True):
                X2 = float(np.dot(x.astype(np.float64), x.astype(np.float64)))
                Y2 = float(np.dot(v.astype(np.float64), v.astype(np.float64))) / 4.0   # v = -2 y'
                X, Y = math.sqrt(X2), math.sqrt(Y2)
                B = pkg.split_lazy_bound(kt, X2, Y2)
                qh, ql, rh, rl = _parts(x, v, flush)
                need = _b_needed(kt, Y2, qh, ql, rh, rl)
                assert need <= B, (kt, name, flush, need, B)
                # the same pair with the signs of the query flipped: cross terms of the other sign
                need_neg = _b_needed(kt, Y2, -qh, -ql, rh, rl)
                assert need_neg <= B, (kt, name, flush, need_neg, B)
                # one concrete accumulation order, every add rounded to fp32
                for sg in (f32(1), f32(-1)):
                    s_hh, s_3 = _lazy_sums_f32(f32(Y2), sg * qh, sg * ql, rh, rl)
                    assert float(s_hh) - float(s_3) <= B, (kt, name, flush, float(s_hh), float(s_3), B)
                # fl(thr + B) in fp32 against the real thr + B_needed, over every threshold a lane can hold
                with np.errstate(over="ignore", under="ignore"):
                    c0, c1, x2 = pkg.tau_consts(kt, X2, Y2, 3)
                    lo, hi = -X2, (X + Y) ** 2 * 1.001 + 1e-30
                    for a in np.concatenate([np.linspace(lo, hi, 17), [0.0, lo, hi]]).astype(f32):
                        dd = f32(a) + f32(x2)
                        thr = f32(a) + f32(f32(1.002) * (f32(c0) + f32(c1) * (dd if dd > 0 else f32(0))))   # tighten
                        thrw = f32(thr + f32(B))
                        assert L(thrw) >= L(thr) + L(max(need, need_neg)), (kt, name, flush, float(a), float(thrw))
                        checked += 1
    assert checked > 1000


def test_bound_is_the_right_size(pkg):
    """At most 2x the worst case measured on parallel vectors with lo parts at their maximum (which attain the
    derivation to within a few per cent), and half of mode 2's c0 (2^-6 XY against 2^-5 XY) + 2 % at unit scale."""
    rng = np.random.default_rng(1)
    for kt in KTS:
        name, x, v = [f for f in _families(rng, kt) if f[0] == "hi_midpoints"][0]
        X2 = float(np.dot(x.astype(np.float64), x.astype(np.float64)))
        Y2 = float(np.dot(v.astype(np.float64), v.astype(np.float64))) / 4.0
        qh, ql, rh, rl = _parts(x, v, False)
        d = lambda t: t.astype(np.float64)   # noqa: E731
        worst = abs(math.fsum(np.concatenate([d(qh) * d(rl), d(ql) * d(rh)])))
        B = pkg.split_lazy_bound(kt, X2, Y2)
        assert worst <= B <= 2.0 * worst, (kt, worst, B)
        assert B <= 1.05 * worst or kt > 128, (kt, worst, B)          # within a few per cent up to KT = 128
        c0 = pkg.tau_consts(kt, 10.7, 10.7, 2)[0]
        Bu = pkg.split_lazy_bound(kt, 10.7, 10.7)
        assert Bu <= 0.5 * c0 * 1.02, (kt, Bu, c0)
        assert Bu >= 2.0 ** -6 * 10.7, (kt, Bu)
    assert pkg.split_lazy_bound(128, 0.0, 0.0) < 1e-29    # zero norms: the 1e-30 constant and the subnormal floor alone


def test_plans_report_the_lazy_schedule_where_enabled(pkg):
    shapes = [(9, 131072, 65537), (16, 250, 31), (17, 65536, 140001), (31, 250, 777), (64, 1000, 50000),
              (64, 65536, 1048576), (100, 65536, 1048576), (128, 65536, 1048576), (128, 200, 5000), (128, 70000, 300001),
              (200, 4096, 300001), (256, 250, 3001), (256, 65536, 1048576)]
    shapes += [(c.k, c.m, c.n) for c in FILTER_CASES if c.dtype == "f32"]
    seen = set()
    for k, m, n in shapes:
        for extra in (0, pkg.NNS_RECORDS_PER_REF):
            d = pkg.plan_filter(k, m, n, flags=extra, schedule=True)
            e = pkg.plan_filter(k, m, n, flags=extra | pkg.NNS_FILTER_SPLIT_EAGER, schedule=True)
            f = pkg.plan_filter(k, m, n, flags=extra | pkg.NNS_FILTER_F32, schedule=True)
            want = int(d["split"] == 1 and d["kt"] in LAZY_KTS and d["tile_rec"] == 0)
            assert d["lazy"] == want, (k, m, n, d)
            assert e["lazy"] == 0 and f["lazy"] == 0 and e["split"] == 1
            assert list(d.values())[:15] == list(e.values())[:15], (k, m, n, d, e)
            seen.add(d["lazy"])
    assert seen == {0, 1}
    assert pkg.plan_filter(128, 65536, 1048576, schedule=True)["lazy"] == 1          # C3
    # callers passing 15 slots see what they saw
    out = np.full(17, -7, np.int32)
    assert pkg.lib.nns_plan_filter(128, 65536, 1048576, 0, 0, out.ctypes.data, 15) == 0
    assert (out[15:] == -7).all()
    p = pkg.plan_filter(128, 65536, 1048576)
    assert "lazy" not in p and list(out[:15]) == list(p.values())


def test_eager_flag_combinations_are_checked(pkg):
    E = pkg.NNS_FILTER_SPLIT_EAGER
    for bf16, flags in ((True, E), (False, E | pkg.NNS_FILTER_F32), (False, E | pkg.NNS_FILTER_BF16),
                        (False, E | pkg.NNS_FILTER_F32 | pkg.NNS_FILTER_BF16)):
        with pytest.raises(pkg.NNSError):
            pkg.plan_filter(128, 1000, 50000, bf16=bf16, flags=flags)
    assert pkg.plan_filter(128, 1000, 50000, flags=E)["split"] == 1


def test_lazy_kernels_isa_is_clean():
    """filter_lazy_kernel<OpLazySplitT<..>>, one per enabled depth: the interval fully unrolled — between the loop header
    and its back-edge exactly the hi-hi MFMAs of a slot (16 hi fragments x 2 query blocks = 32 at KT = 128), the
    refinements laid out behind it — no MFMA read hazards, no scratch."""
    spec = importlib.util.spec_from_file_location("check_mfma_hazards", os.path.join(ROOT, "tools", "check_mfma_hazards.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    with open(chk.compile_isa()) as f:
        text = f.read().splitlines()
    kernels, cur, name = {}, None, None
    for i, l in enumerate(text, 1):
        m = re.match(r"^(_Z\w*filter_lazy_kernel\w*):", l)
        if m:
            name, cur = m.group(1), kernels.setdefault(m.group(1), [])
            continue
        if cur is not None:
            if l.startswith(".Lfunc_end"):
                cur = None
                continue
            cur.append((i, l))
    assert len(kernels) == len(LAZY_KTS), list(kernels)
    for name, lines in kernels.items():
        spb = int(re.search(r"OpLazySplitTILi(\d+)E", name).group(1))   # hi fragments per block = KT / 16
        assert 16 * spb in LAZY_KTS, name
        assert chk.check_kernel(name, lines) == [], name
        assert not any("scratch_" in l for _, l in lines), name
        # every slot loop: header label .. the first branch back to it
        loops = 0
        for idx, (_, l) in enumerate(lines):
            m = re.match(r"^(\.LBB\d+_\d+):.*Loop Header", l)
            if not m:
                continue
            n_mfma, closed = 0, False
            for _, l2 in lines[idx + 1:]:
                if "v_mfma_f32_32x32x16_bf16" in l2:
                    n_mfma += 1
                if re.search(r"s_cbranch_\w+\s+" + re.escape(m.group(1)) + r"\b", l2):
                    closed = True
                    break
            if closed and n_mfma:
                assert n_mfma == 16 * 2, (name, m.group(1), n_mfma)   # 16 hi fragments of a slot x 2 query blocks
                loops += 1
        # (hipcc closes the other interval variants' loops through side blocks; the leading waves' loop is the one laid
        #  out header .. back-edge)
        assert loops >= 1, (name, loops)
        n_all = sum("v_mfma_f32_32x32x16_bf16" in l for _, l in lines)
        assert n_all >= 3 * 32 + 2 * 2 * spb, (name, n_all)   # three interval variants + at least one refinement
