"""CPU tests of the split-bf16 operand form of the MFMA filter (fp32 points; OpSplitT, tau mode 3): the plan picks it by
default at every fp32 depth and NNS_FILTER_F32 turns it off without moving any of the 14 geometry fields; the mode-3
margin covers the split arithmetic — emulated exactly in numpy on adversarial operands (hi / lo rounding midpoints,
cancellation, exponent spread, subnormal and flushed lo parts) — once evaluated in fp32 the way K5 and the filter do;
and the split kernels' ISA passes the hazard / spill checks."""
import importlib.util
import math
import os
import re

import numpy as np
import pytest

from test_filter_cases_cpu import FILTER_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


def _bf16_rne(v):
    """fp32 -> bf16 (round to nearest even) -> fp32, elementwise (finite inputs)."""
    b = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


def _split(v):
    h = _bf16_rne(v)
    lo = _bf16_rne((v - h).astype(np.float32))   # v - h is exact in fp32
    return h, lo


def test_plan_split_by_default_and_f32_flag_keeps_the_geometry(pkg):
    shapes = [(9, 131072, 65537), (16, 250, 31), (17, 65536, 140001), (31, 250, 777), (64, 1000, 50000),
              (100, 65536, 1048576), (128, 65536, 1048576), (128, 200, 5000), (200, 4096, 300001), (256, 250, 3001)]
    shapes += [(c.k, c.m, c.n) for c in FILTER_CASES if c.dtype == "f32"]
    for k, m, n in shapes:
        for extra in (0, pkg.NNS_RECORDS_PER_REF):
            d = pkg.plan_filter(k, m, n, flags=extra)
            f = pkg.plan_filter(k, m, n, flags=extra | pkg.NNS_FILTER_F32)
            assert d["split"] == 1 and f["split"] == 0, (k, m, n, d, f)
            assert {x: v for x, v in d.items() if x != "split"} == {x: v for x, v in f.items() if x != "split"}, (k, m, n)
    # bf16 points and NNS_FILTER_BF16 / k > 256 (bf16 operands) never take the split form
    assert pkg.plan_filter(128, 1000, 50000, bf16=True)["split"] == 0
    assert pkg.plan_filter(128, 1000, 50000, flags=pkg.NNS_FILTER_BF16)["split"] == 0
    assert pkg.plan_filter(300, 1000, 50000)["split"] == 0


def test_plan_filter_fourteen_field_form_unchanged(pkg):
    """Callers that pass 14 slots get exactly the old 14 fields (the 15th is only written when asked for)."""
    out = np.full(16, -7, np.int32)
    assert pkg.lib.nns_plan_filter(128, 65536, 1048576, 0, 0, out.ctypes.data, 14) == 0
    assert (out[14:] == -7).all()
    p = pkg.plan_filter(128, 65536, 1048576)
    assert list(out[:14]) == [p[x] for x in list(p)[:14]]


def _families(rng, kt):
    """(name, x', v) with v = -2 y' (the ref operand): query / ref operands as K2 writes them before the split."""
    f32 = np.float32
    fams = [("uniform", rng.random(kt, dtype=f32) - f32(0.5), (f32(-2) * (rng.random(kt, dtype=f32) - f32(0.5))))]
    # hi rounding midpoints, lo parts as large as they get (|l| = 2^-8 |h|), every product of the same sign
    mid = f32(1.0 + 2.0 ** -8)
    fams.append(("hi_midpoints", np.full(kt, mid, f32), np.full(kt, f32(-2) * mid, f32)))
    # lo rounding midpoints: v - h sits half-way between two bf16 values
    lm = f32(1.0 + 2.0 ** -9 + 2.0 ** -17)
    fams.append(("lo_midpoints", np.full(kt, lm, f32), np.full(kt, f32(-2) * lm, f32)))
    # just off the midpoints, alternating signs, exponent spread over 2^-40 .. 2^40
    e = rng.integers(-40, 40, kt)
    a = np.ldexp(f32(1.0 + 2.0 ** -8 - 2.0 ** -20), e).astype(f32) * np.where(rng.random(kt) < 0.5, f32(-1), f32(1))
    b = np.ldexp(f32(1.0 + 2.0 ** -8 + 2.0 ** -21), -e).astype(f32)
    fams.append(("exponent_spread", a, (f32(-2) * b).astype(f32)))
    # cancellation: x' and v nearly orthogonal (a score near zero against large norms)
    x = rng.standard_normal(kt).astype(f32)
    v = rng.standard_normal(kt).astype(f32)
    v = (v - x * f32(np.dot(x, v) / np.dot(x, x))).astype(f32)
    fams.append(("cancellation", x, v))
    # subnormal lo parts (values near 2^-118: lo ~ 2^-127) and whole operands in the subnormal range
    fams.append(("subnormal_lo", (np.ldexp(f32(1.0 + 2.0 ** -8 + 2.0 ** -20), -118) * np.ones(kt)).astype(f32),
                 (np.ldexp(f32(-1.0 - 2.0 ** -8 - 2.0 ** -21), -117) * np.ones(kt)).astype(f32)))
    fams.append(("subnormal", (rng.random(kt, dtype=f32) * f32(2.0 ** -127)).astype(f32),
                 (rng.random(kt, dtype=f32) * f32(-2.0 ** -126)).astype(f32)))
    return fams


def _split_error(x, v, flush):
    """|x'.v - (qh.rh + qh.rl + ql.rh)| in exact arithmetic (products of fp32 / bf16 values are exact in fp64,
    math.fsum sums them exactly); flush: bf16 parts below 2^-126 read as zero (an MFMA that flushes denormals)."""
    qh, ql = _split(x)
    rh, rl = _split(v)
    if flush:
        qh, ql, rh, rl = (np.where(np.abs(t) < 2.0 ** -126, np.float32(0), t) for t in (qh, ql, rh, rl))
    d = lambda t: t.astype(np.float64)   # noqa: E731
    exact = math.fsum(d(x) * d(v))
    prods = np.concatenate([d(qh) * d(rh), d(qh) * d(rl), d(ql) * d(rh)])
    got = math.fsum(prods)
    return abs(exact - got), float(np.abs(d(x)) @ np.abs(d(v))), math.fsum(np.abs(prods))


def _need3(kt, X2, Y2, a, trunc, sumprod):
    """tau(a) of the proof (finalize.hip) for mode 3, no safety factors, extended precision, with the MEASURED
    truncation of the split and the measured sum of |products| in place of their bounds; the accumulation model
    (2u per add) and the underflow floor as the derivation states them."""
    L = np.longdouble
    X2, Y2 = L(X2) * (1 + 4 * L(U)), L(Y2) * (1 + 4 * L(U))
    X, Y = np.sqrt(X2), np.sqrt(Y2)
    gk = (kt + 2) * L(U) / (1 - (kt + 2) * L(U))
    na = 3 * kt + 3 * (kt // 16) + 2
    gs = 2 * na * L(U) / (1 - 2 * na * L(U))
    # products / adds with results below 2^-126 (flushed or rounded): 2^-126 each; V0's products as in mode 0
    floor = L(3 * kt + na) * L(2.0) ** -126 + L(2 * kt) * L(2.0) ** -150
    e3 = gs * (Y2 + L(sumprod)) + 2 * L(U) * Y2 + L(trunc) + floor
    e2 = L(2.5) * L(U) * (X + Y) ** 2
    return 2 * (e3 + e2) + 2 * gk / (1 - gk) * (max(L(a) + X2, L(0)) + e3 + e2)


def test_tau_mode3_covers_the_split_arithmetic(pkg):
    f32 = np.float32
    L = np.longdouble
    rng = np.random.default_rng(2024)
    checked = 0
    for kt in (16, 32, 64, 128, 256):
        for name, x, v in _families(rng, kt):
            for flush in (False, True):
                trunc, absdot, sumprod = _split_error(x, v, flush)
                X2 = float(np.dot(x.astype(np.float64), x.astype(np.float64)))
                Y2 = float(np.dot(v.astype(np.float64), v.astype(np.float64))) / 4.0   # v = -2 y'
                X, Y = math.sqrt(X2), math.sqrt(Y2)
                # the derivation's truncation bound (relative part + absolute floor for subnormal parts)
                bound = 3 * 2.0 ** -16 * (1 + 2.0 ** -6) * absdot + 2.0 ** -124 * math.sqrt(kt) * (X + 2 * Y)
                assert trunc <= bound, (kt, name, flush, trunc, bound)
                with np.errstate(over="ignore", under="ignore"):
                    c0, c1, x2 = pkg.tau_consts(kt, X2, Y2, 3)
                    lo, hi = -X2, (X + Y) ** 2 * 1.001 + 1e-30
                    for a in np.concatenate([np.linspace(lo, hi, 17), [0.0, lo, hi]]).astype(f32):
                        need = _need3(kt, X2, Y2, float(a), trunc, sumprod)
                        d = f32(a) + f32(x2)
                        tau = f32(c0) + f32(c1) * (d if d > 0 else f32(0))
                        t5 = f32(a) + tau                                      # K5's threshold, in fp32
                        assert L(t5) >= L(a) + need, (kt, name, flush, float(a), float(t5), float(L(a) + need))
                        tf = f32(a) + f32(f32(1.002) * tau)                     # the filter's
                        assert tf >= t5
                        checked += 1
    assert checked > 1000


def test_tau_mode3_between_fp32_and_bf16_operands(pkg):
    """Mode 3's margin is ~2^-13 relative: far below mode 2's (bf16-rounded operands), above mode 0's."""
    for kt in (16, 128, 256):
        t0 = pkg.tau_consts(kt, 10.7, 10.7, 0)[0]
        t2 = pkg.tau_consts(kt, 10.7, 10.7, 2)[0]
        t3 = pkg.tau_consts(kt, 10.7, 10.7, 3)[0]
        assert t0 < t3 < t2 / 16, (kt, t0, t3, t2)


def test_split_kernels_isa_is_clean():
    """The split operators' kernels (filter_split_kernel<OpSplitT<..>>, one per fp32 depth): fully unrolled MFMA
    intervals, no MFMA read hazards, no scratch."""
    spec = importlib.util.spec_from_file_location("check_mfma_hazards", os.path.join(ROOT, "tools", "check_mfma_hazards.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    with open(chk.compile_isa()) as f:
        text = f.read().splitlines()
    kernels, cur = {}, None
    for i, l in enumerate(text, 1):
        m = re.match(r"^(_Z\w*filter_split_kernel\w*):", l)
        if m:
            cur = kernels.setdefault(m.group(1), [])
            continue
        if cur is not None:
            if "s_endpgm" in l:
                cur = None
                continue
            cur.append((i, l))
    assert len(kernels) == 5, list(kernels)   # KT = 16 / 32 / 64 / 128 / 256
    for name, lines in kernels.items():
        assert sum("v_mfma_f32_32x32x16_bf16" in l for _, l in lines) >= 96, name
        assert chk.check_kernel(name, lines) == [], name
        assert not any("scratch_" in l for _, l in lines), name


def test_operand_flags_are_checked(pkg):
    """The operand flags apply to fp32 points and exclude each other: NNS_ERR_INVALID otherwise, as for
    NNS_FILTER_BF16 on bf16 points."""
    for bf16, flags in ((True, pkg.NNS_FILTER_F32), (True, pkg.NNS_FILTER_BF16),
                        (False, pkg.NNS_FILTER_F32 | pkg.NNS_FILTER_BF16)):
        with pytest.raises(pkg.NNSError):
            pkg.plan_filter(128, 1000, 50000, bf16=bf16, flags=flags)
