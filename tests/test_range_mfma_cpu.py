"""CPU tests of the MFMA-filtered range search's boundary (NNS_RANGE_MFMA, K7m): the new symbols and flag, argument
validation before any device is touched, the planner's invariants over a shape grid (batch boundaries included) and the
flag threshold against the mode-3 error terms recomputed here in fp64."""
import ctypes
import json
import math
import os
import re

import numpy as np

from test_range_cpu import NNS_MAX_POINTS, _whole

RANGE_MFMA = 4096
FILTER_BF16, FILTER_F32, SPLIT_EAGER = 128, 1024, 2048
WS_CAP = 256 << 20
LDS_BYTES = 160 * 1024
NEW_SYMBOLS = ("nns_index_range_info", "nns_plan_range_mfma", "nns_range_threshold")
KTS = (16, 32, 64, 128, 256)


def test_symbols_and_flag(pkg):
    raw = ctypes.CDLL(pkg.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in pkg.ABI_SYMBOLS
        assert getattr(raw, name) is not None
    assert pkg.NNS_RANGE_MFMA == RANGE_MFMA
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nns.h")).read()
    assert int(re.search(r"NNS_RANGE_MFMA\s*=\s*(\d+)", header).group(1)) == RANGE_MFMA


def test_unsupported_combinations_before_any_device(pkg):
    L = pkg.lib
    q = np.zeros((4, 16), np.float32)
    lims = np.zeros(5, np.int64)
    qp, lp = q.ctypes.data, lims.ctypes.data
    f32, b16 = L.nns_search_f32_range, L.nns_search_bf16_range
    assert _whole(L, b16, 16, 4, 4, qp, qp, 1.0, lp, flags=RANGE_MFMA) == 5              # bf16 points
    assert _whole(L, f32, 16, 4, 4, qp, qp, 1.0, lp, flags=RANGE_MFMA | FILTER_F32) == 5
    assert _whole(L, f32, 16, 4, 4, qp, qp, 1.0, lp, flags=RANGE_MFMA | FILTER_BF16) == 5
    for k in (1, 7, 257, 1000):
        assert _whole(L, f32, k, 4, 4, qp, qp, 1.0, lp, flags=RANGE_MFMA) == 5, k
    # the flag sets that are unsupported without the flag stay so with it
    for flags in (2, 3, 32, 128, 256, 512, 1 << 30):
        assert _whole(L, f32, 16, 4, 4, qp, qp, 1.0, lp, flags=flags | RANGE_MFMA) == 5, flags
    # index creation: the same combinations, before the device is looked for
    h = ctypes.c_void_p()
    assert L.nns_index_create_bf16(ctypes.byref(h), 0, 16, 4, qp, 0, RANGE_MFMA, None) == 5
    assert L.nns_index_create(ctypes.byref(h), 0, 16, 4, qp, 0, RANGE_MFMA | FILTER_F32, None) == 5
    assert L.nns_index_create(ctypes.byref(h), 0, 16, 4, qp, 0, RANGE_MFMA | FILTER_BF16, None) == 5
    assert L.nns_index_create(ctypes.byref(h), 0, 7, 4, qp, 0, RANGE_MFMA, None) == 5
    assert L.nns_index_create(ctypes.byref(h), 0, 257, 4, qp, 0, RANGE_MFMA, None) == 5
    assert not h
    out = np.zeros(4, np.int64)
    assert L.nns_index_range_info(None, out.ctypes.data, 4) == 1


def test_existing_validation_holds_with_the_flag(pkg):
    L = pkg.lib
    q = np.zeros((4, 16), np.float32)
    lims = np.zeros(5, np.int64)
    qp, lp = q.ctypes.data, lims.ctypes.data
    fn, F = L.nns_search_f32_range, RANGE_MFMA
    assert _whole(L, fn, 16, 0, 4, qp, qp, 1.0, lp, flags=F) == 1
    assert _whole(L, fn, 16, -1, 4, qp, qp, 1.0, lp, flags=F) == 1
    assert _whole(L, fn, 16, 4, 0, qp, qp, 1.0, lp, flags=F) == 1
    assert _whole(L, fn, 0, 4, 4, qp, qp, 1.0, lp, flags=F) == 1
    assert _whole(L, fn, -2, 4, 4, qp, qp, 1.0, lp, flags=F) == 1
    assert _whole(L, fn, 16, 4, 4, None, qp, 1.0, lp, flags=F) == 1
    assert _whole(L, fn, 16, 4, 4, qp, None, 1.0, lp, flags=F) == 1
    assert _whole(L, fn, 16, 4, 4, qp, qp, 1.0, None, flags=F) == 1
    assert _whole(L, fn, 16, 4, 4, qp, qp, 1.0, lp, flags=F, idx=False) == 1
    assert _whole(L, fn, 16, 4, 4, qp, qp, float("nan"), lp, flags=F) == 1
    assert _whole(L, fn, 16, 4, 4, qp, qp, -1.0, lp, flags=F) == 1
    assert b"radius2" in L.nns_last_error()
    assert _whole(L, fn, 16, 4, NNS_MAX_POINTS + 1, qp, qp, 1.0, lp, flags=F) == 1
    assert _whole(L, fn, 16, NNS_MAX_POINTS + 1, 4, qp, qp, 1.0, lp, flags=F) == 1
    assert _whole(L, fn, 16385, 4, 4, qp, qp, 1.0, lp, flags=F) == 5


def test_plan_range_mfma_invariants(pkg):
    batched = 0
    for k in (8, 16, 17, 64, 128, 129, 256):
        for m in (64, 65, 513, 4096, 65536, 1 << 20):
            for n in (33, 1000, 70000, 1 << 20, 1 << 24):
                for flags in (0, SPLIT_EAGER):
                    p = pkg.plan_range_mfma(k, m, n, flags)
                    f = pkg.plan_filter(k, m, n, flags=flags, schedule=True)
                    where = (k, m, n, flags, p)
                    assert p["kt"] == f["kt"] and p["block_refs"] == 32, where
                    blocks = p["blocks_per_query"]
                    assert blocks * 32 == f["n_pad"] >= n, where
                    assert (blocks - 1) * 32 < n + f["slot_pts"], where      # at most one ring slot of padding
                    assert 0 < p["flag_ws_bytes"] <= WS_CAP, where
                    batch, batches = p["batch"], p["batches"]
                    assert batch % f["queries_per_wg"] == 0, where
                    assert batches * batch >= m and (batches - 1) * batch < m, where      # every batch non-empty
                    assert p["flag_ws_bytes"] == batch * -(-blocks // 32) * 4, where
                    assert p["grid_x"] * f["queries_per_wg"] == batch, where
                    assert 1 <= p["grid_y"] <= f["total_slots"], where
                    assert p["lds_bytes"] <= LDS_BYTES, where
                    # the lazy image layout exactly where the 1-NN filter of such an index keeps it (the lazy depths,
                    # unless the eager flag is given; plan_filter's "lazy" at a long stream says which depths those are)
                    lazy_depth = pkg.plan_filter(k, 65536, 1 << 20, flags=0, schedule=True)["lazy"] == 1
                    assert p["layout"] == int(lazy_depth and not flags), where
                    batched += batches > 1
    assert batched > 0                                                       # the grid reaches the batched plans
    # a batch boundary by hand: 2^20 queries x 70000 refs at k = 8 is 69 words per query: two batches
    p = pkg.plan_range_mfma(8, 1 << 20, 70000)
    assert p["batches"] == 2 and p["batch"] % 512 == 0 and p["batch"] * 69 * 4 <= WS_CAP < (p["batch"] + 512) * 69 * 4


def test_plans_are_the_parents(pkg, golden_dir):
    """nns_plan_range_mfma over the grid of test_plan_range_mfma_invariants, and the two rejected depths: all ten
    values and the status codes recorded from the commit before the planner took its geometry, its split chooser
    and its workspace cap from the shared definitions."""
    with open(os.path.join(golden_dir, "range_mfma_plans_parent.json")) as f:
        want = {(e["k"], e["m"], e["n"], e["flags"]): (e["status"], e["plan"]) for e in json.load(f)}
    out = np.zeros(10, np.int32)
    shapes = [(k, m, n, flags) for k in (8, 16, 17, 64, 128, 129, 256) for m in (64, 65, 513, 4096, 65536, 1 << 20)
              for n in (33, 1000, 70000, 1 << 20, 1 << 24) for flags in (0, SPLIT_EAGER)]
    shapes += [(7, 64, 1000, 0), (257, 64, 1000, 0)]
    assert len(shapes) == 422 and set(shapes) == set(want)
    for k, m, n, flags in shapes:
        out[:] = -1
        status = pkg.lib.nns_plan_range_mfma(k, m, n, flags, out.ctypes.data, 10)
        plan = [int(v) for v in out] if status == 0 else None
        assert (status, plan) == want[(k, m, n, flags)], (k, m, n, flags, status, plan, want[(k, m, n, flags)])
    assert want[(7, 64, 1000, 0)] == (5, None) and want[(257, 64, 1000, 0)] == (5, None)


def test_plan_range_mfma_rejects(pkg):
    out = np.zeros(10, np.int32)
    L = pkg.lib
    assert L.nns_plan_range_mfma(7, 64, 1000, 0, out.ctypes.data, 10) == 5
    assert L.nns_plan_range_mfma(257, 64, 1000, 0, out.ctypes.data, 10) == 5
    assert L.nns_plan_range_mfma(16, 64, 1000, FILTER_F32, out.ctypes.data, 10) == 5
    assert L.nns_plan_range_mfma(16, 64, 1000, FILTER_BF16, out.ctypes.data, 10) == 5
    assert L.nns_plan_range_mfma(16, 64, 1000, 0, out.ctypes.data, 9) == 1
    assert L.nns_plan_range_mfma(16, 0, 1000, 0, out.ctypes.data, 10) == 1
    assert L.nns_plan_range_mfma(16, 64, NNS_MAX_POINTS + 1, 0, out.ctypes.data, 10) == 1


def _mode3_errors(kt, qnorm2, ymax2):
    """e3 + e2 of tau_consts' mode 3 (nns_internal.h), in fp64."""
    u = 2.0 ** -24
    X2 = float(qnorm2) * (1 + 4 * u)
    Y2 = float(ymax2) * (1 + 4 * u)
    X, Y = math.sqrt(X2), math.sqrt(Y2)
    na = 3.0 * kt + 3.0 * (kt // 16) + 2.0
    gs = 2 * na * u / (1 - 2 * na * u)
    et = 3.0 * 2.0 ** -15 * (1 + 2.0 ** -6) * X * Y
    ef = 2.0 ** -124 * math.sqrt(kt) * (X + 2 * Y) + (7.0 * kt + 4) * 2.0 ** -126
    e3 = gs * (Y2 + (1 + 2.0 ** -5) * 2 * X * Y) + 2 * u * Y2 + et + ef
    e2 = 2.5 * u * (X + Y) ** 2
    return e3 + e2


def test_range_threshold_covers_the_model_and_is_monotone(pkg):
    rng = np.random.default_rng(5)
    for scale in (1.0, 2.0 ** -120, 2.0 ** 80):          # squared norms of data at unit, 2^-60 and 2^40 scale
        for kt in KTS:
            for _ in range(40):
                qn, ym, r2 = (np.float32(v * scale) for v in rng.random(3) * (4.0, 4.0, 8.0))
                thr = pkg.range_threshold(kt, float(qn), float(ym), float(r2))
                assert thr >= (float(r2) - float(qn)) + _mode3_errors(kt, qn, ym), (scale, kt, qn, ym, r2, thr)
                # monotone in radius2: neighbouring floats and a larger step
                up = np.nextafter(r2, np.float32(np.inf))
                assert pkg.range_threshold(kt, float(qn), float(ym), float(up)) >= thr
                assert pkg.range_threshold(kt, float(qn), float(ym), float(r2 * np.float32(1.5))) >= thr
    # a radius far beyond the cloud: the roundings relative to radius2 are covered too
    thr = pkg.range_threshold(64, 1.0, 1.0, 1e30)
    assert thr >= 1e30
    assert pkg.range_threshold(64, 1.0, 1.0, 3.4e38) == float("inf") or pkg.range_threshold(64, 1.0, 1.0, 3.4e38) >= 3.4e38
