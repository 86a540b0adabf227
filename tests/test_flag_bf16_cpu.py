"""CPU tests of the MFMA-filtered range and top-K searches for bf16 points (NNS_RANGE_MFMA / NNS_TOPK_MFMA on a bf16
index, 32 <= k <= 256): the new symbols, the planners' invariants over a shape grid against the bf16 filter's geometry,
what is rejected and what no longer is (up to the device lookup), and the flag threshold against the mode-1 error terms
recomputed here in fp64."""
import ctypes
import math

import numpy as np

from test_range_cpu import NNS_MAX_POINTS

RANGE_MFMA, TOPK_MFMA = 4096, 8192
FILTER_BF16, FILTER_F32, SPLIT_EAGER = 128, 1024, 2048
WS_CAP = 256 << 20
LDS_BYTES = 160 * 1024
NEW_SYMBOLS = ("nns_plan_range_mfma_bf16", "nns_plan_topk_mfma_bf16", "nns_range_threshold_bf16")
RANGE_FIELDS = ("kt", "block_refs", "blocks_per_query", "batch", "batches", "flag_ws_bytes", "grid_x", "grid_y",
                "lds_bytes", "layout")
KS = (32, 40, 128, 129, 256)
MS = (64, 65, 513, 65536, 1 << 20)
NS = (33, 1000, 70000, 1 << 20, 1 << 24)


def test_symbols(pkg):
    raw = ctypes.CDLL(pkg.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in pkg.ABI_SYMBOLS
        assert getattr(raw, name) is not None


def _check_range_fields(pkg, p, k, m, n, where):
    """test_plan_range_mfma_invariants' assertions (test_range_mfma_cpu.py), against the bf16 filter's geometry"""
    f = pkg.plan_filter(k, m, n, bf16=True)
    assert p["kt"] == f["kt"] == (128 if k <= 128 else 256) and p["block_refs"] == 32, where
    blocks = p["blocks_per_query"]
    assert blocks * 32 == f["n_pad"] >= n, where
    assert (blocks - 1) * 32 < n + f["slot_pts"], where                  # at most one ring slot of padding
    assert f["slot_pts"] == 32 * 32 * 16 // p["kt"], where               # a slot: 32 KiB of the image, 4 or 2 blocks
    assert 0 < p["flag_ws_bytes"] <= WS_CAP, where
    batch, batches = p["batch"], p["batches"]
    assert batch % f["queries_per_wg"] == 0, where
    assert batches * batch >= m and (batches - 1) * batch < m, where      # every batch non-empty
    assert p["flag_ws_bytes"] == batch * -(-blocks // 32) * 4, where
    assert p["grid_x"] * f["queries_per_wg"] == batch, where
    assert 1 <= p["grid_y"] <= f["total_slots"], where
    assert p["lds_bytes"] <= LDS_BYTES, where
    assert p["layout"] == 2, where                                       # the order-1 16x16x32 image
    return batches


def test_plan_range_mfma_bf16_invariants(pkg):
    batched = 0
    for k in KS:
        for m in MS:
            for n in NS:
                p = pkg.plan_range_mfma(k, m, n, bf16=True)
                batched += _check_range_fields(pkg, p, k, m, n, (k, m, n, p)) > 1
    assert batched > 0                                                       # the grid reaches the batched plans
    # a batch boundary by hand: 4096 queries x (2^24 + 1) refs at k = 32 is 16385 words per query: two batches
    p = pkg.plan_range_mfma(32, 4096, (1 << 24) + 1, bf16=True)
    assert p["batches"] == 2 and p["batch"] % 512 == 0
    assert p["batch"] * 16385 * 4 <= WS_CAP < (p["batch"] + 512) * 16385 * 4


def test_plan_topk_mfma_bf16_invariants(pkg):
    """test_plan_topk_mfma_invariants' assertions (test_topk_mfma_cpu.py) on the bf16 plan"""
    taken = fallen = chunked = 0
    out = np.zeros(10, np.int32)
    for k in KS:
        for m in (1, 63) + MS:
            for n in NS + (6000, 70001):
                for kn in (1, 10, 100, 256):
                    p = pkg.plan_topk_mfma(k, m, n, kn, bf16=True)
                    where = (k, m, n, kn, p)
                    blocks = -(-n // 32)
                    sb0, sb = (max(math.isqrt(-(-kn * n * w16 // 512) - 1) + 1, -(-max(2048, 16 * kn) // 32))
                               for w16 in (16, max(k, 16)))
                    if sb > blocks // 2:
                        sb = max(sb0, blocks // 2)
                    stride = blocks // sb
                    assert p["stride"] == stride, where
                    step = max(stride, 1)
                    assert p["sample_blocks"] == -(-blocks // step), where
                    last = (p["sample_blocks"] - 1) * step * 32
                    assert last < n, where
                    assert p["sample_refs"] == (p["sample_blocks"] - 1) * 32 + min(32, n - last), where
                    assert p["sample_refs"] <= n, where
                    if stride >= 2:
                        assert p["sample_blocks"] >= sb and p["sample_refs"] >= max(kn, 2017), where
                    ok = pkg.lib.nns_plan_range_mfma_bf16(k, m, n, 0, out.ctypes.data, 10) == 0
                    assert p["filtered"] == int(stride >= 2 and m >= 64 and ok), where
                    assert 0 < p["select_lds_bytes"] <= 64 * 1024, where
                    if not p["filtered"]:
                        fallen += 1
                        assert all(p[f] == 0 for f in RANGE_FIELDS + ("chunks", "chunk_words")), where
                        continue
                    taken += 1
                    r = pkg.plan_range_mfma(k, m, n, bf16=True)
                    assert all(p[f] == r[f] for f in RANGE_FIELDS), where
                    _check_range_fields(pkg, p, k, m, n, where)
                    wpq = -(-p["blocks_per_query"] // 32)
                    assert p["chunk_words"] % 64 == 0 and p["chunks"] >= 1, where
                    assert p["chunks"] * p["chunk_words"] >= wpq > (p["chunks"] - 1) * p["chunk_words"], where
                    if m >= 4096:
                        assert p["chunks"] == 1, where
                    chunked += p["chunks"] > 1
    assert taken > 100 and fallen > 100 and chunked > 0


def test_plan_rejects(pkg):
    L = pkg.lib
    out = np.zeros(17, np.int32)
    op = out.ctypes.data
    for k in (16, 31, 257):
        assert L.nns_plan_range_mfma_bf16(k, 64, 100000, 0, op, 10) == 5, k
        assert L.nns_plan_topk_mfma_bf16(k, 64, 100000, 4, 0, op, 17) == 5, k
    for flags in (FILTER_F32, FILTER_BF16, SPLIT_EAGER):                     # the flags of fp32 points, as nns_plan_filter
        assert L.nns_plan_filter(64, 64, 100000, 1, flags, op, 16) == 1, flags
        assert L.nns_plan_range_mfma_bf16(64, 64, 100000, flags, op, 10) == 1, flags
        assert L.nns_plan_topk_mfma_bf16(64, 64, 100000, 4, flags, op, 17) == 1, flags
    assert L.nns_plan_range_mfma_bf16(64, 64, 100000, 0, op, 9) == 1
    assert L.nns_plan_range_mfma_bf16(64, 0, 100000, 0, op, 10) == 1
    assert L.nns_plan_range_mfma_bf16(64, 64, NNS_MAX_POINTS + 1, 0, op, 10) == 1
    assert L.nns_plan_range_mfma_bf16(64, 64, 100000, 0, None, 10) == 1
    assert L.nns_plan_topk_mfma_bf16(64, 64, 100000, 257, 0, op, 17) == 5
    assert L.nns_plan_topk_mfma_bf16(64, 64, 100000, 0, 0, op, 17) == 1
    assert L.nns_plan_topk_mfma_bf16(64, 64, 100000, 4, 0, op, 16) == 1
    for k in (32, 256):
        assert L.nns_plan_range_mfma_bf16(k, 64, 100000, 0, op, 10) == 0, k
        assert L.nns_plan_topk_mfma_bf16(k, 64, 100000, 4, 0, op, 17) == 0, k
    # the fp32 plans are what they were: k = 16 plans, the layout field stays 0 / 1
    assert L.nns_plan_range_mfma(16, 64, 100000, 0, op, 10) == 0 and out[9] == 0
    assert L.nns_plan_range_mfma(128, 64, 100000, 0, op, 10) == 0 and out[9] == 1
    assert L.nns_plan_range_mfma(128, 64, 100000, FILTER_BF16, op, 10) == 5


def _calls(L, k, flags_range, flags_topk, device):
    """Status of index creation and of the two whole calls for bf16 points at depth k (4 queries, 4 refs)."""
    pts = np.zeros((4, k), np.uint16)
    lims = np.zeros(5, np.int64)
    idx = np.zeros(16, np.int32)
    pp = pts.ctypes.data
    h = ctypes.c_void_p()
    pidx = ctypes.POINTER(ctypes.c_int)()
    out = {}
    out["create_range"] = L.nns_index_create_bf16(ctypes.byref(h), device, k, 4, pp, 0, flags_range, None)
    assert not h
    out["create_topk"] = L.nns_index_create_bf16(ctypes.byref(h), device, k, 4, pp, 0, flags_topk, None)
    assert not h
    out["range"] = L.nns_search_bf16_range(k, 4, 4, pp, pp, 1.0, lims.ctypes.data, ctypes.byref(pidx), None, flags_range,
                                           device)
    assert not pidx
    out["topk"] = L.nns_search_bf16_topk(k, 4, 4, pp, pp, 4, idx.ctypes.data, None, 1, flags_topk, device)
    return out


def test_bf16_points_rejected_outside_32_to_256(pkg):
    L = pkg.lib
    for k in (16, 31, 257):
        assert set(_calls(L, k, RANGE_MFMA, TOPK_MFMA, 0).values()) == {5}, k
    # the operand flags of fp32 points stay unsupported with either flag
    for extra in (FILTER_F32, FILTER_BF16):
        assert set(_calls(L, 64, RANGE_MFMA | extra, TOPK_MFMA | extra, 0).values()) == {5}, extra


def test_bf16_points_accepted_up_to_the_device_lookup(pkg):
    """At k = 32 and 256 neither flag is rejected any more: with device -1 every call gets as far as looking for its
    device (no device: 4; a device, but not that one: 1) and says so."""
    L = pkg.lib
    for k in (32, 256):
        for name, status in _calls(L, k, RANGE_MFMA, TOPK_MFMA, -1).items():
            assert status in (1, 4), (k, name, status)
        assert b"device" in L.nns_last_error().lower()


def _mode1_errors(kt, qnorm2, ymax2):
    """e3 (+ e2 = 0: no centring) of tau_consts' mode 1 (nns_internal.h), in fp64."""
    u = 2.0 ** -24
    X2 = float(qnorm2) * (1 + 4 * u)
    Y2 = float(ymax2) * (1 + 4 * u)
    X, Y = math.sqrt(X2), math.sqrt(Y2)
    na = kt + kt // 16 + 2
    gf = 2 * na * u / (1 - 2 * na * u)
    return gf * (Y2 + 2 * X * Y) + 2 * u * Y2


def test_range_threshold_bf16_covers_the_model_and_is_monotone(pkg):
    rng = np.random.default_rng(6)
    for scale in (1.0, 2.0 ** -120, 2.0 ** 80):          # squared norms of data at unit, 2^-60 and 2^40 scale
        for kt in (128, 256):
            for _ in range(40):
                qn, ym, r2 = (np.float32(v * scale) for v in rng.random(3) * (4.0, 4.0, 8.0))
                thr = pkg.range_threshold(kt, float(qn), float(ym), float(r2), bf16=True)
                assert thr >= (float(r2) - float(qn)) + _mode1_errors(kt, qn, ym), (scale, kt, qn, ym, r2, thr)
                up = np.nextafter(r2, np.float32(np.inf))
                assert pkg.range_threshold(kt, float(qn), float(ym), float(up), bf16=True) >= thr
                assert pkg.range_threshold(kt, float(qn), float(ym), float(r2 * np.float32(1.5)), bf16=True) >= thr
                # exact operands: never a wider margin than the split form's at the same depth and norms
                assert thr <= pkg.range_threshold(kt, float(qn), float(ym), float(r2))
    thr = pkg.range_threshold(128, 1.0, 1.0, 1e30, bf16=True)
    assert thr >= 1e30
    big = pkg.range_threshold(128, 1.0, 1.0, 3.4e38, bf16=True)
    assert big == float("inf") or big >= 3.4e38
    out = np.zeros(1, np.float32)
    assert pkg.lib.nns_range_threshold_bf16(0, 1.0, 1.0, 1.0, out.ctypes.data) == 1
    assert pkg.lib.nns_range_threshold_bf16(128, 1.0, 1.0, 1.0, None) == 1
