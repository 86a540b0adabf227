"""CPU tests of the MFMA-filtered top-K search's boundary (NNS_TOPK_MFMA, K6m): the new symbols and flag, argument
validation before any device is touched, and the planner's invariants over a grid of (k, m, n, kn): the block sample
of the bound scan, when the filtered path is taken, and the selection's chunks."""
import ctypes
import math
import os
import re

import numpy as np

from test_topk_cpu import NNS_MAX_POINTS

TOPK_MFMA = 8192
FILTER_BF16, FILTER_F32, SPLIT_EAGER = 128, 1024, 2048
NEW_SYMBOLS = ("nns_index_topk_info", "nns_plan_topk_mfma")
RANGE_FIELDS = ("kt", "block_refs", "blocks_per_query", "batch", "batches", "flag_ws_bytes", "grid_x", "grid_y",
                "lds_bytes", "layout")


def test_symbols_and_flag(pkg):
    raw = ctypes.CDLL(pkg.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in pkg.ABI_SYMBOLS
        assert getattr(raw, name) is not None
    assert pkg.NNS_TOPK_MFMA == TOPK_MFMA
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nns.h")).read()
    assert int(re.search(r"NNS_TOPK_MFMA\s*=\s*(\d+)", header).group(1)) == TOPK_MFMA
    # a bit of its own among the flags
    others = [int(v) for v in re.findall(r"NNS_[A-Z0-9_]+\s*=\s*(\d+),?\s*/\*", header)]
    assert others.count(TOPK_MFMA) == 1


def test_unsupported_combinations_before_any_device(pkg):
    L = pkg.lib
    q = np.zeros((4, 16), np.float32)
    idx = np.zeros(4 * 4, np.int32)
    qp, ip = q.ctypes.data, idx.ctypes.data
    f32, b16 = L.nns_search_f32_topk, L.nns_search_bf16_topk
    assert b16(16, 4, 4, qp, qp, 4, ip, None, 1, TOPK_MFMA, 0) == 5                      # bf16 points
    assert f32(16, 4, 4, qp, qp, 4, ip, None, 1, TOPK_MFMA | FILTER_F32, 0) == 5
    assert f32(16, 4, 4, qp, qp, 4, ip, None, 1, TOPK_MFMA | FILTER_BF16, 0) == 5
    for k in (1, 7, 257, 1000):
        assert f32(k, 4, 4, qp, qp, 4, ip, None, 1, TOPK_MFMA, 0) == 5, k
    # the flag sets that are unsupported without the flag stay so with it
    for flags in (2, 3, 32, 128, 256, 512, 4096, 1 << 30):
        assert f32(16, 4, 4, qp, qp, 4, ip, None, 1, flags | TOPK_MFMA, 0) == 5, flags
    # index creation: the same combinations, before the device is looked for
    h = ctypes.c_void_p()
    assert L.nns_index_create_bf16(ctypes.byref(h), 0, 16, 4, qp, 0, TOPK_MFMA, None) == 5
    assert L.nns_index_create(ctypes.byref(h), 0, 16, 4, qp, 0, TOPK_MFMA | FILTER_F32, None) == 5
    assert L.nns_index_create(ctypes.byref(h), 0, 16, 4, qp, 0, TOPK_MFMA | FILTER_BF16, None) == 5
    assert L.nns_index_create(ctypes.byref(h), 0, 7, 4, qp, 0, TOPK_MFMA, None) == 5
    assert L.nns_index_create(ctypes.byref(h), 0, 257, 4, qp, 0, TOPK_MFMA, None) == 5
    assert not h
    out = np.zeros(4, np.int64)
    assert L.nns_index_topk_info(None, out.ctypes.data, 4) == 1


def test_existing_validation_holds_with_the_flag(pkg):
    L = pkg.lib
    q = np.zeros((4, 16), np.float32)
    idx = np.zeros(4 * 300, np.int32)
    qp, ip = q.ctypes.data, idx.ctypes.data
    fn, F = L.nns_search_f32_topk, TOPK_MFMA
    assert fn(16, 4, 4, qp, qp, 0, ip, None, 1, F, 0) == 1
    assert fn(16, 4, 4, qp, qp, -3, ip, None, 1, F, 0) == 1
    assert fn(16, 4, 4, qp, qp, 257, ip, None, 1, F, 0) == 5
    assert b"above 256" in L.nns_last_error()
    assert fn(16, 0, 4, qp, qp, 4, ip, None, 1, F, 0) == 1
    assert fn(16, -1, 4, qp, qp, 4, ip, None, 1, F, 0) == 1
    assert fn(16, 4, 0, qp, qp, 4, ip, None, 1, F, 0) == 1
    assert fn(0, 4, 4, qp, qp, 4, ip, None, 1, F, 0) == 1
    assert fn(16, 4, 4, qp, qp, 4, None, None, 1, F, 0) == 1
    assert fn(16, 4, 4, None, qp, 4, ip, None, 1, F, 0) == 1
    assert fn(16, 4, 4, qp, None, 4, ip, None, 1, F, 0) == 1
    assert fn(16, 4, NNS_MAX_POINTS + 1, qp, qp, 4, ip, None, 1, F, 0) == 1
    assert b"NNS_MAX_POINTS" in L.nns_last_error()
    assert fn(16, NNS_MAX_POINTS + 1, 4, qp, qp, 4, ip, None, 1, F, 0) == 1
    assert fn(16385, 4, 4, qp, qp, 4, ip, None, 1, F, 0) == 5


def test_plan_topk_mfma_rejects(pkg):
    out = np.zeros(17, np.int32)
    L, op = pkg.lib, out.ctypes.data
    assert L.nns_plan_topk_mfma(7, 64, 100000, 4, 0, op, 17) == 5
    assert L.nns_plan_topk_mfma(257, 64, 100000, 4, 0, op, 17) == 5
    assert L.nns_plan_topk_mfma(16, 64, 100000, 4, FILTER_F32, op, 17) == 5
    assert L.nns_plan_topk_mfma(16, 64, 100000, 4, FILTER_BF16, op, 17) == 5
    assert L.nns_plan_topk_mfma(16, 64, 100000, 257, 0, op, 17) == 5
    assert L.nns_plan_topk_mfma(16, 64, 100000, 0, 0, op, 17) == 1
    assert L.nns_plan_topk_mfma(16, 64, 100000, 4, 0, op, 16) == 1
    assert L.nns_plan_topk_mfma(16, 0, 100000, 4, 0, op, 17) == 1
    assert L.nns_plan_topk_mfma(16, 64, NNS_MAX_POINTS + 1, 4, 0, op, 17) == 1
    assert L.nns_plan_topk_mfma(16, 64, 100000, 4, 0, None, 17) == 1


def _range_plan_ok(pkg, k, m, n, flags):
    out = np.zeros(10, np.int32)
    return pkg.lib.nns_plan_range_mfma(k, m, n, flags, out.ctypes.data, 10) == 0


def test_plan_topk_mfma_invariants(pkg):
    taken = fallen = chunked = 0
    for k in (8, 17, 128, 256):
        for m in (1, 63, 64, 600, 4096, 1 << 20):
            for n in (33, 6000, 70001, 140000, 1 << 20, 1 << 24):
                for kn in (1, 10, 100, 256):
                    for flags in (0, SPLIT_EAGER):
                        p = pkg.plan_topk_mfma(k, m, n, kn, flags)
                        where = (k, m, n, kn, flags, p)
                        blocks = -(-n // 32)
                        # the sample rule
                        # (the smallest s with 512 s^2 >= kn n w16, and the floor of 2048 or 16 kn refs; w16 = max(k, 16):
                        #  a selected ref weighs k / 16 scanned ones, but never so that a stride of 2 is lost)
                        sb0, sb = (max(math.isqrt(-(-kn * n * w16 // 512) - 1) + 1, -(-max(2048, 16 * kn) // 32))
                                   for w16 in (16, max(k, 16)))
                        if sb > blocks // 2:
                            sb = max(sb0, blocks // 2)
                        stride = blocks // sb
                        assert p["stride"] == stride, where
                        step = max(stride, 1)
                        # whole blocks, evenly spaced, the last one starts below n; at least kn refs
                        assert p["sample_blocks"] == -(-blocks // step), where
                        last = (p["sample_blocks"] - 1) * step * 32
                        assert last < n, where
                        assert p["sample_refs"] == (p["sample_blocks"] - 1) * 32 + min(32, n - last), where
                        assert p["sample_refs"] <= n, where
                        if stride >= 2:
                            assert p["sample_blocks"] >= sb and p["sample_refs"] >= max(kn, 2017), where
                        # filtered exactly when there is something to skip, enough queries, and a flag-pass plan
                        ok = _range_plan_ok(pkg, k, m, n, flags)
                        assert p["filtered"] == int(stride >= 2 and m >= 64 and ok), where
                        assert 0 < p["select_lds_bytes"] <= 64 * 1024, where
                        if not p["filtered"]:
                            fallen += 1
                            assert all(p[f] == 0 for f in RANGE_FIELDS + ("chunks", "chunk_words")), where
                            continue
                        taken += 1
                        r = pkg.plan_range_mfma(k, m, n, flags)
                        assert all(p[f] == r[f] for f in RANGE_FIELDS), where
                        # the chunks cover all flag words, none is empty, each is whole 64-word steps
                        wpq = -(-p["blocks_per_query"] // 32)
                        assert p["chunk_words"] % 64 == 0 and p["chunks"] >= 1, where
                        assert p["chunks"] * p["chunk_words"] >= wpq > (p["chunks"] - 1) * p["chunk_words"], where
                        if m >= 4096:
                            assert p["chunks"] == 1, where
                        chunked += p["chunks"] > 1
    assert taken > 100 and fallen > 100 and chunked > 0
    # by hand: n = 140000, kn = 256 -> sqrt(256 * 140000 / 32) = 1058.3: 1059 blocks of 4375, stride 4
    p = pkg.plan_topk_mfma(16, 64, 140000, 256)
    assert (p["stride"], p["sample_blocks"], p["filtered"]) == (4, 1094, 1)
    # kn = 1: the 2048-ref floor, 64 blocks
    p = pkg.plan_topk_mfma(16, 64, 6000, 1)
    assert (p["stride"], p["sample_blocks"], p["sample_refs"], p["filtered"]) == (2, 94, 3008, 1)
    # too few refs for the sample: K6
    assert pkg.plan_topk_mfma(16, 64, 4000, 1)["filtered"] == 0
    assert pkg.plan_topk_mfma(16, 63, 140000, 10)["filtered"] == 0
