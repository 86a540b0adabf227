"""CPU tests of uint8 points (dtype code 5): the new entry points exist and host.py declares their arguments, the plans
are int8's field for field, the flag-pass plans are the bf16 ones at depth 128 in everything but the depth and the
layout, create and the whole calls answer their flag checks before any device is looked up, the exact flag threshold
(nns_range_threshold_u8) agrees with integer arithmetic, and the compiled flag kernel (range_flag_u8_kernel: RmU8Tile on
v_mfma_i32_16x16x64_i8 through the compiler builtin) has no spills and no private segment."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, 1, 5
I8, U8 = 3, 5   # the bf16_points / dtype values of int8 and uint8 points
MFMA_I8 = "v_mfma_i32_16x16x64_i8"
SYMBOLS = ("nns_index_create_u8", "nns_index_search_u8", "nns_search_u8_ex", "nns_search_u8_topk", "nns_search_u8_range",
           "nns_plan_range_mfma_u8", "nns_plan_topk_mfma_u8", "nns_range_threshold_u8")


def test_the_uint8_symbols_exist_and_have_argtypes(pkg):
    raw = ctypes.CDLL(pkg.LIB_PATH)
    for name in SYMBOLS:
        assert getattr(raw, name) is not None
        assert name in pkg.ABI_SYMBOLS
        assert getattr(pkg.lib, name).argtypes, name
        assert getattr(pkg.lib, name).restype is ctypes.c_int, name
    twins = {"nns_index_create_u8": "nns_index_create_i8", "nns_index_search_u8": "nns_index_search_i8",
             "nns_search_u8_ex": "nns_search_i8_ex", "nns_search_u8_topk": "nns_search_i8_topk",
             "nns_search_u8_range": "nns_search_i8_range", "nns_plan_range_mfma_u8": "nns_plan_range_mfma_bf16",
             "nns_plan_topk_mfma_u8": "nns_plan_topk_mfma_bf16"}
    for new, old in twins.items():
        assert list(getattr(pkg.lib, new).argtypes) == list(getattr(pkg.lib, old).argtypes), new
    for name in ("search_u8", "search_topk_u8", "search_range_u8", "to_u8"):
        assert callable(getattr(pkg, name))


@pytest.mark.parametrize("k", [3, 32, 33, 100, 128, 129, 256])
def test_plans_at_dtype_5_equal_int8s(pkg, k):
    for m, n in ((64, 2048), (130, 5003), (4096, 1 << 20)):
        if k >= 32:
            for flags in (0, pkg.NNS_RECORDS_PER_REF):
                got = pkg.plan_filter(k, m, n, bf16=U8, flags=flags, schedule=True)
                assert got == pkg.plan_filter(k, m, n, bf16=I8, flags=flags, schedule=True), (k, m, n, flags)
                assert got["kt"] == 256 and got["lpq"] == 4
        for kn in (1, 10, 100):
            assert pkg.plan_topk(k, m, n, kn, bf16=U8) == pkg.plan_topk(k, m, n, kn, bf16=I8)
        assert pkg.plan_range(k, m, n, bf16=U8) == pkg.plan_range(k, m, n, bf16=I8)


def test_plan_filter_rejections(pkg):
    out = np.zeros(16, np.int32)
    L = pkg.lib
    assert L.nns_plan_filter(256, 64, 2048, U8, 0, out.ctypes.data, 16) == OK
    assert L.nns_plan_filter(257, 64, 2048, U8, 0, out.ctypes.data, 16) == UNSUPPORTED
    for flag in (pkg.NNS_FILTER_BF16, pkg.NNS_FILTER_F32, pkg.NNS_FILTER_SPLIT_EAGER):
        assert L.nns_plan_filter(128, 64, 2048, U8, flag, out.ctypes.data, 16) == INVALID, flag
    assert L.nns_plan_filter(128, 64, 2048, U8, pkg.NNS_REFS_SOA, out.ctypes.data, 16) == UNSUPPORTED
    for flag in (pkg.NNS_RANGE_MFMA, pkg.NNS_TOPK_MFMA):
        assert L.nns_plan_filter(128, 64, 2048, U8, flag, out.ctypes.data, 16) == OK, flag
        assert L.nns_plan_filter(128, 64, 2048, I8, flag, out.ctypes.data, 16) == UNSUPPORTED, flag   # (int8: as before)
    assert L.nns_plan_filter(0, 64, 2048, U8, 0, out.ctypes.data, 16) == INVALID


@pytest.mark.parametrize("k", [32, 40, 64, 100, 128, 129, 200, 256])
def test_flag_plans_are_the_bf16_plans_at_depth_128(pkg, k):
    """A uint8 block (2 ref tiles x 4 k-steps of 64 bytes) has the bytes of the 128-deep bf16 block: every field of the
    flag-pass plans but the depth and the layout is that plan's, whatever k <= 256 is."""
    kb = min(k, 128)   # (any k of the 128-deep bf16 tile plans alike)
    for m, n in ((130, 2999), (600, 70001), (4096, 1 << 20)):
        got = pkg.plan_range_mfma(k, m, n, bf16=U8)
        want = pkg.plan_range_mfma(kb, m, n, bf16=True)
        assert want["kt"] == 128 and want["layout"] == 2
        assert got["kt"] == 256 and got["layout"] == 3
        skip = ("kt", "layout")
        assert {f: v for f, v in got.items() if f not in skip} == {f: v for f, v in want.items() if f not in skip}, (k, m, n)
        # the block bytes: fragments per block (kt / 64 x 2 tiles x 1 KiB against kt / 32 x 2 x 1 KiB)
        assert got["kt"] // 64 == want["kt"] // 32 == 4
        for kn in (1, 10, 100):
            g = pkg.plan_topk_mfma(k, m, n, kn, bf16=U8)
            # (the sample rule weighs k: compare with the bf16 plan at the same k where it is 128-deep)
            w = pkg.plan_topk_mfma(k, m, n, kn, bf16=True)
            assert {f: g[f] for f in ("sample_blocks", "stride", "sample_refs", "filtered", "select_lds_bytes")} == \
                   {f: w[f] for f in ("sample_blocks", "stride", "sample_refs", "filtered", "select_lds_bytes")}
            if g["filtered"]:
                assert g["kt"] == 256 and g["layout"] == 3
                w128 = pkg.plan_topk_mfma(kb, m, n, kn, bf16=True)
                if w128["filtered"]:
                    same = ("block_refs", "blocks_per_query", "batch", "batches", "flag_ws_bytes", "grid_x", "grid_y",
                            "lds_bytes", "chunks", "chunk_words")
                    assert {f: g[f] for f in same} == {f: w128[f] for f in same}, (k, m, n, kn)
    out = np.zeros(17, np.int32)
    L = pkg.lib
    for kbad in (31, 257):
        assert L.nns_plan_range_mfma_u8(kbad, 130, 2999, 0, out.ctypes.data, 10) == UNSUPPORTED
        assert L.nns_plan_topk_mfma_u8(kbad, 130, 70001, 10, 0, out.ctypes.data, 17) == UNSUPPORTED
    for flag in (pkg.NNS_FILTER_F32, pkg.NNS_FILTER_BF16, pkg.NNS_FILTER_SPLIT_EAGER):
        assert L.nns_plan_range_mfma_u8(64, 130, 2999, flag, out.ctypes.data, 10) == INVALID
        assert L.nns_plan_topk_mfma_u8(64, 130, 70001, 10, flag, out.ctypes.data, 17) == INVALID
    assert L.nns_plan_range_mfma_u8(64, 130, 2999, 0, out.ctypes.data, 9) == INVALID


def test_create_and_whole_calls_reject_flags_before_the_device_lookup(pkg):
    L = pkg.lib
    pts = np.zeros((4, 64), np.uint8)
    big = np.zeros((4, 300), np.uint8)
    pp, pb = pts.ctypes.data, big.ctypes.data
    h = ctypes.c_void_p()
    idx = np.zeros((4, 2), np.int32)
    lims = np.zeros(5, np.int64)
    pidx = ctypes.POINTER(ctypes.c_int)()
    # (device 99 does not exist anywhere: a device lookup would answer NNS_ERR_NODEVICE or NNS_ERR_INVALID with another text)
    calls = {
        "create": lambda flag, k=64, p=pp: L.nns_index_create_u8(ctypes.byref(h), 99, k, 4, p, 0, flag, None),
        "ex": lambda flag, k=64, p=pp: L.nns_search_u8_ex(k, 4, 4, p, p, idx.ctypes.data, None, 1, flag, 99),
        "topk": lambda flag, k=64, p=pp: L.nns_search_u8_topk(k, 4, 4, p, p, 2, idx.ctypes.data, None, 1, flag, 99),
        "range": lambda flag, k=64, p=pp: L.nns_search_u8_range(k, 4, 4, p, p, 1.0, lims.ctypes.data, ctypes.byref(pidx), None,
                                                                flag, 99),
    }
    i8pre = (getattr(pkg, "NNS_FILTER_I8PRE_OFF", 0), getattr(pkg, "NNS_FILTER_I8PRE_FORCE", 0))
    assert all(i8pre), i8pre
    for name, call in calls.items():
        for flag in (pkg.NNS_FILTER_BF16, pkg.NNS_FILTER_F32, pkg.NNS_FILTER_SPLIT_EAGER) + i8pre:
            assert call(flag) == INVALID, (name, flag)
            assert b"uint8" in L.nns_last_error() and b"operand flags" in L.nns_last_error(), (name, L.nns_last_error())
        assert call(pkg.NNS_REFS_SOA) == UNSUPPORTED, name
        assert b"uint8" in L.nns_last_error(), (name, L.nns_last_error())
        assert call(pkg.NNS_PATH_MFMA, 300, pb) == UNSUPPORTED, name          # no tile beyond k = 256
        assert b"uint8" in L.nns_last_error(), (name, L.nns_last_error())
        for flag in (pkg.NNS_RANGE_MFMA, pkg.NNS_TOPK_MFMA):                   # the flag passes outside 32 .. 256
            for k, p in ((300, pb), (16, pp)):
                assert call(flag, k, p) == UNSUPPORTED, (name, flag, k)
                assert b"uint8" in L.nns_last_error(), (name, L.nns_last_error())
        assert b"NNS_" not in L.nns_last_error()
        assert not h and not pidx
    assert L.nns_search_u8_topk(64, 4, 4, pp, pp, 300, idx.ctypes.data, None, 1, 0, 99) == UNSUPPORTED
    # int8 points keep their answers
    p8 = np.zeros((4, 64), np.int8).ctypes.data
    for flag in (pkg.NNS_RANGE_MFMA, pkg.NNS_TOPK_MFMA):
        assert L.nns_index_create_i8(ctypes.byref(h), 99, 64, 4, p8, 0, flag, None) == UNSUPPORTED


def test_null_and_non_positive_arguments(pkg):
    L = pkg.lib
    pts = np.zeros((4, 64), np.uint8)
    pp = pts.ctypes.data
    h = ctypes.c_void_p()
    idx = np.zeros((4, 2), np.int32)
    lims = np.zeros(5, np.int64)
    pidx = ctypes.POINTER(ctypes.c_int)()
    assert L.nns_index_create_u8(None, 0, 64, 4, pp, 0, 0, None) == INVALID
    assert L.nns_index_create_u8(ctypes.byref(h), 0, 64, 4, None, 0, 0, None) == INVALID
    assert L.nns_index_create_u8(ctypes.byref(h), 0, 0, 4, pp, 0, 0, None) == INVALID
    assert L.nns_index_create_u8(ctypes.byref(h), 0, 64, 0, pp, 0, 0, None) == INVALID
    assert L.nns_index_search_u8(None, 4, pp, pp, None) == INVALID
    assert L.nns_search_u8_ex(64, 0, 4, pp, pp, idx.ctypes.data, None, 1, 0, 0) == INVALID
    assert L.nns_search_u8_ex(64, 4, 4, None, pp, idx.ctypes.data, None, 1, 0, 0) == INVALID
    assert L.nns_search_u8_topk(64, 4, 4, pp, pp, 0, idx.ctypes.data, None, 1, 0, 0) == INVALID
    assert L.nns_search_u8_range(64, 4, 4, pp, pp, 1.0, lims.ctypes.data, None, None, 0, 0) == INVALID
    assert L.nns_search_u8_range(64, 4, 4, pp, pp, -1.0, lims.ctypes.data, ctypes.byref(pidx), None, 0, 0) == INVALID
    assert L.nns_range_threshold_u8(1.0, 1.0, None) == INVALID
    assert not h and not pidx


def test_to_u8_takes_uint8_only(pkg):
    a = np.array([[0, 255, 128, 5]], np.uint8)
    assert pkg.to_u8(a).dtype == np.uint8 and np.array_equal(pkg.to_u8(a), a)
    for other in (np.int8, np.int16, np.float32, np.uint16):
        with pytest.raises(ValueError):
            pkg.to_u8(a.astype(other))
    with pytest.raises(ValueError):
        pkg.to_u8(a[0])
    with pytest.raises(ValueError):
        pkg.to_u8(a[None])


def test_the_exact_threshold_against_integer_arithmetic(pkg):
    """s <= thr  <=>  qnorm2 + s <= radius2, exactly, for the integer scores of attainable distances in a band round each
    threshold (and at the ends of the score range)."""
    from fractions import Fraction
    checked = 0
    for qn in (0, 1, 2 ** 22 - 1, 2 ** 22):
        for r2 in (0.0, 0.5, 1.0, 16646399.5, 16646400.0, float(2 ** 24), 1e30):
            r2 = float(np.float32(r2))   # (the radius the C ABI receives is an fp32: 16 646 399.5 arrives as its neighbour)
            thr = pkg.range_threshold_u8(float(qn), r2)
            assert thr == float(np.float32(thr)) and thr == int(thr)
            centre = int(min(Fraction(r2), Fraction(2 ** 24))) - qn          # integer arithmetic
            top = 16646400 - qn                                               # the score of the largest distance
            band = list(range(centre - 40, centre + 41)) + list(range(top - 40, top + 1)) + [-qn, 0]
            for s in band:
                # (what the tile can see: a score is the integer d - qnorm2 of a distance d = 0 .. 256 * 255^2 < 2^24; beyond
                #  that the clamp of the radius to 2^24 has nothing to agree with)
                if abs(s) >= 2 ** 24 or not 0 <= qn + s <= 16646400:
                    continue
                sf = np.float32(s)
                assert int(sf) == s
                assert bool(sf <= np.float32(thr)) == (Fraction(qn + s) <= Fraction(r2)), (qn, r2, s, thr)
                checked += 1
    assert checked > 1500


# ---- the compiled kernel -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flag_isa():
    """The ISA listing (a list of lines) of one device-only compilation of range_mfma.hip."""
    out = os.path.join(tempfile.mkdtemp(prefix="nns_isa_"), "range_mfma.s")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
           "-fno-slp-vectorize", "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only", "-o", out,
           os.path.join(ROOT, "nns-cuda_amd", "csrc", "range_mfma.hip")]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(out) as f:
        return f.read().splitlines()


def _kernel_bodies(text, which):
    """{mangled name: lines from the kernel's label to its s_endpgm} of the kernels whose name matches `which`"""
    found, name = {}, None
    for line in text:
        m = re.match(r"^(_Z\w*)\s*:", line)
        if m and name is None and re.search(which, m.group(1)):
            name = m.group(1)
            found[name] = []
        elif name is not None:
            found[name].append(line)
            if "s_endpgm" in line:
                name = None
    return found


def test_the_u8_flag_kernel_has_no_spills_and_no_private_segment(flag_isa):
    kernels = _kernel_bodies(flag_isa, r"range_flag_u8_kernel")
    assert len(kernels) == 1, list(kernels)
    joined = "\n".join(flag_isa)
    for name, lines in kernels.items():
        n8 = sum(MFMA_I8 in l for l in lines)
        print(f"{name}: {n8} {MFMA_I8}")
        assert n8 >= 32, name                                      # (a block: 4 k-steps x 4 query tiles x 2 ref tiles)
        assert not any("v_mfma_f32" in l for l in lines), name
        meta = re.search(r"\.name:\s+" + re.escape(name) + r"\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", joined)
        assert meta, name
        assert int(meta.group(1)) == 0, name
        seg = re.search(r"\.name:\s+" + re.escape(name) + r"\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", joined)
        assert seg, name
        assert int(seg.group(1)) == 0, name
    # the earlier flag kernels are the seven they were: five split depths, two bf16 depths
    assert len(_kernel_bodies(flag_isa, r"range_flag_kernel")) == 5
    assert len(_kernel_bodies(flag_isa, r"range_flag16_kernel")) == 2
