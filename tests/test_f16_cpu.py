"""CPU tests of fp16 points: the five entry points exist, the filter plans fp16 points exactly as bf16 points at the two
16x16x32 depths and refuses what is not built, create answers its flag checks before any device is looked up, tau mode 4
behaves, and the compiled f16 filter kernels (filter_f16_kernel: OpF16T at KT = 128 and 256) are free of MFMA read
hazards and spills."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, 1, 5
F16 = 2   # the bf16_points / dtype value of fp16 points
MFMA_F16 = "v_mfma_f32_16x16x32_f16"


def test_the_five_fp16_symbols_exist(pkg):
    raw = ctypes.CDLL(pkg.LIB_PATH)
    for name in ("nns_index_create_f16", "nns_index_search_f16", "nns_search_f16_ex", "nns_search_f16_topk",
                 "nns_search_f16_range"):
        assert getattr(raw, name) is not None
        assert name in pkg.ABI_SYMBOLS


@pytest.mark.parametrize("k", [32, 100, 128, 129, 256])
def test_plan_geometry_is_the_bf16_one_field_for_field(pkg, k):
    for m, n in ((64, 2048), (130, 5003), (4096, 1 << 20)):
        for flags in (0, pkg.NNS_RECORDS_PER_REF):
            want = pkg.plan_filter(k, m, n, bf16=True, flags=flags, schedule=True)
            got = pkg.plan_filter(k, m, n, bf16=F16, flags=flags, schedule=True)
            assert got == want, (k, m, n, flags)
            assert got["kt"] == (128 if k <= 128 else 256) and got["lpq"] == 4
    # the exact scans share one geometry between the 16-bit types
    assert pkg.plan_topk(k, 70, 3000, 10, bf16=F16) == pkg.plan_topk(k, 70, 3000, 10, bf16=True)
    assert pkg.plan_range(k, 70, 3000, bf16=F16) == pkg.plan_range(k, 70, 3000, bf16=True)


def test_plan_rejections(pkg):
    out = np.zeros(16, np.int32)
    L = pkg.lib
    assert L.nns_plan_filter(256, 64, 2048, F16, 0, out.ctypes.data, 16) == OK
    assert L.nns_plan_filter(257, 64, 2048, F16, 0, out.ctypes.data, 16) == UNSUPPORTED
    assert L.nns_plan_filter(257, 64, 2048, 1, 0, out.ctypes.data, 16) == OK      # (bf16 points keep their deep tiles)
    for flag in (pkg.NNS_FILTER_BF16, pkg.NNS_FILTER_F32, pkg.NNS_FILTER_SPLIT_EAGER):
        assert L.nns_plan_filter(128, 64, 2048, F16, flag, out.ctypes.data, 16) == INVALID, flag
    for flag in (pkg.NNS_RANGE_MFMA, pkg.NNS_TOPK_MFMA):
        assert L.nns_plan_filter(128, 64, 2048, F16, flag, out.ctypes.data, 16) == UNSUPPORTED, flag


def test_create_and_whole_calls_reject_flags_before_the_device_lookup(pkg):
    L = pkg.lib
    pts = np.zeros((4, 64), np.uint16)
    pp = pts.ctypes.data
    h = ctypes.c_void_p()
    # (device 99 does not exist anywhere: a device lookup would answer NNS_ERR_NODEVICE or NNS_ERR_INVALID with another text)
    for flag in (pkg.NNS_RANGE_MFMA, pkg.NNS_TOPK_MFMA):
        assert L.nns_index_create_f16(ctypes.byref(h), 99, 64, 4, pp, 0, flag, None) == UNSUPPORTED, flag
        assert b"fp16" in L.nns_last_error()
        assert not h
    for flag in (pkg.NNS_FILTER_BF16, pkg.NNS_FILTER_F32, pkg.NNS_FILTER_SPLIT_EAGER):
        assert L.nns_index_create_f16(ctypes.byref(h), 99, 64, 4, pp, 0, flag, None) == INVALID, flag
        assert b"operand flags" in L.nns_last_error()
        assert not h
    idx = np.zeros((4, 2), np.int32)
    assert L.nns_search_f16_topk(64, 4, 4, pp, pp, 2, idx.ctypes.data, None, 1, pkg.NNS_TOPK_MFMA, 99) == UNSUPPORTED
    assert L.nns_search_f16_topk(64, 4, 4, pp, pp, 300, idx.ctypes.data, None, 1, 0, 99) == UNSUPPORTED
    lims = np.zeros(5, np.int64)
    pidx = ctypes.POINTER(ctypes.c_int)()
    assert L.nns_search_f16_range(64, 4, 4, pp, pp, 1.0, lims.ctypes.data, ctypes.byref(pidx), None, pkg.NNS_RANGE_MFMA,
                                  99) == UNSUPPORTED
    assert not pidx
    # argument checks of the new entry points, as their bf16 twins'
    assert L.nns_index_create_f16(None, 0, 64, 4, pp, 0, 0, None) == INVALID
    assert L.nns_index_search_f16(None, 4, pp, pp, None) == INVALID
    assert L.nns_search_f16_ex(64, 0, 4, pp, pp, idx.ctypes.data, None, 1, 0, 0) == INVALID


def test_tau_consts_mode_4(pkg):
    out = np.zeros(3, np.float32)
    assert pkg.lib.nns_tau_consts(128, 1.0, 1.0, 5, out.ctypes.data) == INVALID
    prev = None
    for kt in (128, 256):
        for x2, y2 in ((1.0, 1.0), (40.0, 90.0), (1e-6, 3e4), (0.0, 0.0)):
            c0, c1, xx = pkg.tau_consts(kt, x2, y2, 4)
            assert c0 > 0 and c1 > 0 and xx >= x2
            # exact operands: not above the split operands' margin, and mode 1's formula unless the per-add allowance
            # was raised
            c0_3, c1_3, _ = pkg.tau_consts(kt, x2, y2, 3)
            assert c0 <= c0_3 and c1 <= c1_3
            c0_1, c1_1, _ = pkg.tau_consts(kt, x2, y2, 1)
            assert c0 >= c0_1 and c1 == c1_1
        cur = pkg.tau_consts(kt, 40.0, 90.0, 4)
        if prev is not None:
            assert cur[0] > prev[0] and cur[1] > prev[1]   # monotone in kt
        prev = cur


def test_to_f16_bits_takes_float16_or_bit_patterns_only(pkg):
    a = np.array([[1.0, -2.0, 6.1e-5, 65504.0]], np.float16)
    bits = pkg.to_f16_bits(a)
    assert bits.dtype == np.uint16 and np.array_equal(bits, a.view(np.uint16))
    assert np.array_equal(pkg.to_f16_bits(bits), bits)
    with pytest.raises(ValueError):
        pkg.to_f16_bits(a.astype(np.float32))
    with pytest.raises(ValueError):
        pkg.to_f16_bits(bits[0])


# ---- the compiled kernels ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def isa():
    """(checker module, {name: lines} of the f16 filter kernels, whole text) of one compilation of filter_mfma.hip."""
    spec = importlib.util.spec_from_file_location("check_mfma_hazards", os.path.join(ROOT, "tools", "check_mfma_hazards.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    with open(chk.compile_isa()) as f:
        text = f.read().splitlines()
    return chk, chk.split_kernels(text, r"filter_f16_kernel"), text


def test_two_f16_filter_kernels_clean_of_hazards_and_spills(isa):
    chk, kernels, text = isa
    assert chk.WAITS[MFMA_F16] == 8
    assert len(kernels) == 2, list(kernels)
    joined = "\n".join(text)
    for name, lines in kernels.items():
        n16 = sum(MFMA_F16 in l for _, l in lines)
        print(f"{name}: {n16} {MFMA_F16}")
        assert n16 >= 64, name                                   # (every interval is fully unrolled: 32 steps)
        assert not any("v_mfma_f32_16x16x32_bf16" in l for _, l in lines), name
        assert chk.check_kernel(name, lines) == [], name
        assert not any("scratch_" in l for _, l in lines), name
        # the kernel's metadata entry
        meta = re.search(r"\.name:\s+" + re.escape(name) + r"\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", joined)
        assert meta, name
        assert int(meta.group(1)) == 0, name
    # the bf16 kernels kept their mnemonic and the whole-file check sees the new kernels too
    allk = chk.split_kernels(text)
    assert set(kernels) <= set(allk)
    assert sum("filter_kernel" in k for k in allk) == 12


def test_checker_flags_an_early_read_after_an_f16_mfma(isa):
    chk, _, _ = isa
    early = """
    v_mfma_f32_16x16x32_f16 v[178:181], v[232:235], v[62:65], v[178:181]
    v_mfma_f32_16x16x32_f16 v[170:173], v[232:235], v[94:97], v[170:173]
    v_min3_f32 v163, v185, v178, v179
    """
    assert len(chk.check_kernel("k", list(enumerate(early.splitlines(), 1)))) == 1
    ok = """
    v_mfma_f32_16x16x32_f16 v[178:181], v[232:235], v[62:65], v[178:181]
    v_mfma_f32_16x16x32_f16 v[178:181], v[236:239], v[66:69], v[178:181]
    s_nop 7
    v_min3_f32 v163, v185, v178, v179
    """
    assert chk.check_kernel("k", list(enumerate(ok.splitlines(), 1))) == []
