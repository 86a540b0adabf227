"""CPU tests of int8 points: the five entry points exist, the filter plans int8 points on the geometry of the 128-deep
bf16 tile at depth 256 and refuses what is not built, create and the three whole calls answer their flag checks before any
device is looked up, and the compiled int8 filter kernel (filter_i8_kernel: OpI8 on v_mfma_i32_16x16x64_i8 through the
compiler builtin) has no scratch accesses and no spills."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, 1, 5
I8 = 3   # the bf16_points / dtype value of int8 points
MFMA_I8 = "v_mfma_i32_16x16x64_i8"
SYMBOLS = ("nns_index_create_i8", "nns_index_search_i8", "nns_search_i8_ex", "nns_search_i8_topk", "nns_search_i8_range")


def test_the_five_int8_symbols_exist(pkg):
    raw = ctypes.CDLL(pkg.LIB_PATH)
    for name in SYMBOLS:
        assert getattr(raw, name) is not None
        assert name in pkg.ABI_SYMBOLS
    assert pkg.lib.nns_version() == 1


@pytest.mark.parametrize("k", [32, 100, 128, 129, 256])
def test_filter_plan_reuses_the_128_deep_bf16_geometry_at_depth_256(pkg, k):
    """An int8 block (2 ref tiles x 4 k-steps of 64 dims x 1 byte) has the bytes and fragments of the 128-deep bf16 block
    (2 x 4 k-steps of 32 dims x 2 bytes): every field but the depth is that plan's, whatever k <= 256 is."""
    for m, n in ((64, 2048), (4096, 1 << 20)):
        for flags in (0, pkg.NNS_RECORDS_PER_REF):
            got = pkg.plan_filter(k, m, n, bf16=I8, flags=flags, schedule=True)
            kt = got["kt"]
            assert kt >= k and kt % 64 == 0 and kt <= 256, (k, kt)
            # the bf16 plan whose blocks have the int8 blocks' bytes: depth kt / 2 (any k of that tile plans alike)
            want = pkg.plan_filter(kt // 2, m, n, bf16=True, flags=flags, schedule=True)
            assert want["kt"] == kt // 2
            assert {f: v for f, v in got.items() if f != "kt"} == {f: v for f, v in want.items() if f != "kt"}, (k, m, n, flags)
            assert got["lpq"] == 4
    assert pkg.plan_topk(k, 70, 3000, 10, bf16=I8) == pkg.plan_topk(k, 70, 3000, 10, bf16=True)
    assert pkg.plan_range(k, 70, 3000, bf16=I8) == pkg.plan_range(k, 70, 3000, bf16=True)


def test_plan_rejections(pkg):
    out = np.zeros(16, np.int32)
    L = pkg.lib
    assert L.nns_plan_filter(256, 64, 2048, I8, 0, out.ctypes.data, 16) == OK
    assert L.nns_plan_filter(257, 64, 2048, I8, 0, out.ctypes.data, 16) == UNSUPPORTED
    for flag in (pkg.NNS_FILTER_BF16, pkg.NNS_FILTER_F32, pkg.NNS_FILTER_SPLIT_EAGER):
        assert L.nns_plan_filter(128, 64, 2048, I8, flag, out.ctypes.data, 16) == INVALID, flag
    for flag in (pkg.NNS_RANGE_MFMA, pkg.NNS_TOPK_MFMA, pkg.NNS_REFS_SOA):
        assert L.nns_plan_filter(128, 64, 2048, I8, flag, out.ctypes.data, 16) == UNSUPPORTED, flag
    # no tau mode 5, and the other selftest modes' argument checks are what they were (host only: before any device)
    assert L.nns_tau_consts(256, 1.0, 1.0, 5, out.ctypes.data) == INVALID
    assert L.nns_plan_filter(0, 64, 2048, I8, 0, out.ctypes.data, 16) == INVALID
    assert L.nns_plan_filter(64, 64, 2048, I8, 0, None, 16) == INVALID


def test_create_and_whole_calls_reject_flags_before_the_device_lookup(pkg):
    L = pkg.lib
    pts = np.zeros((4, 64), np.int8)
    pp = pts.ctypes.data
    h = ctypes.c_void_p()
    idx = np.zeros((4, 2), np.int32)
    lims = np.zeros(5, np.int64)
    pidx = ctypes.POINTER(ctypes.c_int)()
    # (device 99 does not exist anywhere: a device lookup would answer NNS_ERR_NODEVICE or NNS_ERR_INVALID with another text)
    calls = {
        "create": lambda flag: L.nns_index_create_i8(ctypes.byref(h), 99, 64, 4, pp, 0, flag, None),
        "ex": lambda flag: L.nns_search_i8_ex(64, 4, 4, pp, pp, idx.ctypes.data, None, 1, flag, 99),
        "topk": lambda flag: L.nns_search_i8_topk(64, 4, 4, pp, pp, 2, idx.ctypes.data, None, 1, flag, 99),
        "range": lambda flag: L.nns_search_i8_range(64, 4, 4, pp, pp, 1.0, lims.ctypes.data, ctypes.byref(pidx), None, flag, 99),
    }
    for name, call in calls.items():
        for flag in (pkg.NNS_RANGE_MFMA, pkg.NNS_TOPK_MFMA, pkg.NNS_REFS_SOA):
            assert call(flag) == UNSUPPORTED, (name, flag)
            assert b"int8" in L.nns_last_error(), (name, L.nns_last_error())
        for flag in (pkg.NNS_FILTER_BF16, pkg.NNS_FILTER_F32, pkg.NNS_FILTER_SPLIT_EAGER):
            assert call(flag) == INVALID, (name, flag)
            assert b"operand flags" in L.nns_last_error(), (name, L.nns_last_error())
        assert b"NNS_" not in L.nns_last_error()
        assert not h and not pidx
    assert L.nns_index_create_i8(ctypes.byref(h), 99, 300, 4, pp, 0, pkg.NNS_RANGE_MFMA, None) == UNSUPPORTED
    assert L.nns_search_i8_topk(64, 4, 4, pp, pp, 300, idx.ctypes.data, None, 1, 0, 99) == UNSUPPORTED


def test_null_and_non_positive_arguments(pkg):
    L = pkg.lib
    pts = np.zeros((4, 64), np.int8)
    pp = pts.ctypes.data
    h = ctypes.c_void_p()
    idx = np.zeros((4, 2), np.int32)
    lims = np.zeros(5, np.int64)
    pidx = ctypes.POINTER(ctypes.c_int)()
    assert L.nns_index_create_i8(None, 0, 64, 4, pp, 0, 0, None) == INVALID
    assert L.nns_index_create_i8(ctypes.byref(h), 0, 64, 4, None, 0, 0, None) == INVALID
    assert L.nns_index_create_i8(ctypes.byref(h), 0, 0, 4, pp, 0, 0, None) == INVALID
    assert L.nns_index_create_i8(ctypes.byref(h), 0, 64, 0, pp, 0, 0, None) == INVALID
    assert L.nns_index_create_i8(ctypes.byref(h), 0, 64, -3, pp, 0, 0, None) == INVALID
    assert L.nns_index_search_i8(None, 4, pp, pp, None) == INVALID
    assert L.nns_search_i8_ex(64, 0, 4, pp, pp, idx.ctypes.data, None, 1, 0, 0) == INVALID
    assert L.nns_search_i8_ex(64, 4, 4, None, pp, idx.ctypes.data, None, 1, 0, 0) == INVALID
    assert L.nns_search_i8_ex(64, 4, 4, pp, pp, None, None, 1, 0, 0) == INVALID
    assert L.nns_search_i8_ex(-1, 4, 4, pp, pp, idx.ctypes.data, None, 1, 0, 0) == INVALID
    assert L.nns_search_i8_topk(64, 4, 0, pp, pp, 2, idx.ctypes.data, None, 1, 0, 0) == INVALID
    assert L.nns_search_i8_topk(64, 4, 4, pp, None, 2, idx.ctypes.data, None, 1, 0, 0) == INVALID
    assert L.nns_search_i8_topk(64, 4, 4, pp, pp, 0, idx.ctypes.data, None, 1, 0, 0) == INVALID
    assert L.nns_search_i8_range(64, 4, 4, pp, pp, 1.0, lims.ctypes.data, None, None, 0, 0) == INVALID
    assert L.nns_search_i8_range(64, 0, 4, pp, pp, 1.0, lims.ctypes.data, ctypes.byref(pidx), None, 0, 0) == INVALID
    assert L.nns_search_i8_range(64, 4, 4, pp, pp, -1.0, lims.ctypes.data, ctypes.byref(pidx), None, 0, 0) == INVALID
    assert not h and not pidx


def test_to_i8_takes_int8_only(pkg):
    a = np.array([[-128, 127, 0, 5]], np.int8)
    assert pkg.to_i8(a).dtype == np.int8 and np.array_equal(pkg.to_i8(a), a)
    with pytest.raises(ValueError):
        pkg.to_i8(a.astype(np.int16))
    with pytest.raises(ValueError):
        pkg.to_i8(a[0])


# ---- the compiled kernel -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def isa():
    """(checker module, {name: lines} of the int8 filter kernel, whole text) of one compilation of filter_mfma.hip."""
    spec = importlib.util.spec_from_file_location("check_mfma_hazards", os.path.join(ROOT, "tools", "check_mfma_hazards.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    with open(chk.compile_isa()) as f:
        text = f.read().splitlines()
    return chk, chk.split_kernels(text, r"filter_i8_kernel"), text


def test_the_i8_filter_kernel_has_no_scratch_and_no_spills(isa):
    chk, kernels, text = isa
    assert len(kernels) == 1, list(kernels)
    joined = "\n".join(text)
    for name, lines in kernels.items():
        n8 = sum(MFMA_I8 in l for _, l in lines)
        print(f"{name}: {n8} {MFMA_I8}")
        assert n8 >= 128, name                                   # (every interval is fully unrolled: 32 steps x 4 query tiles)
        assert not any("v_mfma_f32" in l for _, l in lines), name
        assert not any("scratch_" in l for _, l in lines), name
        meta = re.search(r"\.name:\s+" + re.escape(name) + r"\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", joined)
        assert meta, name
        assert int(meta.group(1)) == 0, name
    # the new kernel is not an instantiation of filter_kernel<>: the bf16 / fp32 kernels are the twelve they were
    assert sum("filter_kernel" in k for k in chk.split_kernels(text)) == 12
