"""What every point type refuses, and with which words: (status, nns_last_error()) of the create, whole-call and plan
entry points over all six dtypes, every flag bit of include/nns.h (and the pairs the library names) and the k values
around every tile limit, held against a recording of the library as it was before the point-type table
(tests/golden/point_type_rules.json).  The calls name device 99: one that passes every argument check ends at the device
lookup, is recorded as "DEVICE" and compared with what a plain fp32 call answers for device 99 on the running machine,
so the grid holds with and without a GPU.

The recording is written by record() below from a library given by NNS_LIB_PATH (a build of the commit to record):
    NNS_LIB_PATH=/path/to/libnns_mi355x.so python tests/test_point_type_rules_cpu.py
"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "point_type_rules.json")

INFIX = ("f32", "bf16", "f16", "i8", "b1", "u8")   # by dtype code 0 .. 5
B1 = 4
# 0, every flag bit of include/nns.h, the pairs the library's checks name
BITS = (1, 2, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768)
PAIRS = (128 | 1024, 2048 | 128, 16384 | 32768, 4096 | 1024, 8192 | 128)
FLAGS = (0,) + BITS + PAIRS
KS = (7, 8, 31, 32, 256, 257, 1024, 1025)
KS_B1 = (64, 8192, 8224, 33)   # bits; 33: not whole words
M = N = 4
DEVICE = 99
SENTINEL = "nns_keys_topk_merge: m must be > 0 and pointers non-null (m=0)"


def _ks(dtype):
    return KS_B1 if dtype == B1 else KS


def _calls(pkg):
    """(name, dtypes, takes flags, f(dtype, k, flags) -> status) of every entry point of the grid."""
    L = pkg.lib
    buf = np.zeros(4 * 1025 * 4 + 64, np.uint8)   # 4 points of the widest row, 4-byte aligned
    assert buf.ctypes.data % 4 == 0
    q = r = buf.ctypes.data
    idx = np.zeros(16, np.int32)
    dist = np.zeros(16, np.float32)
    lims = np.zeros(M + 1, np.int64)
    out = np.zeros(32, np.int32)
    o = out.ctypes.data
    all_dt = range(6)

    def create(dt, k, flags):
        h = ctypes.c_void_p()
        fn = getattr(L, "nns_index_create" + ("" if dt == 0 else "_" + INFIX[dt]))
        rc = fn(ctypes.byref(h), DEVICE, k, N, r, 0, flags, None)
        assert rc != 0 and not h.value
        return rc

    def ex(dt, k, flags):
        return getattr(L, f"nns_search_{INFIX[dt]}_ex")(k, M, N, q, r, idx.ctypes.data, dist.ctypes.data, 1, flags, DEVICE)

    def topk(dt, k, flags):
        return getattr(L, f"nns_search_{INFIX[dt]}_topk")(k, M, N, q, r, 1, idx.ctypes.data, dist.ctypes.data, 1, flags, DEVICE)

    def rng(dt, k, flags):
        pidx = ctypes.POINTER(ctypes.c_int)()
        pdist = ctypes.POINTER(ctypes.c_float)()
        rc = getattr(L, f"nns_search_{INFIX[dt]}_range")(k, M, N, q, r, 1.0, lims.ctypes.data, ctypes.byref(pidx),
                                                         ctypes.byref(pdist), flags, DEVICE)
        assert rc != 0 and not pidx and not pdist
        return rc

    def mfma_plan(base, nout, with_kn):
        def f(dt, k, flags):
            fn = getattr(L, base + {0: "", 1: "_bf16", 5: "_u8"}[dt])
            return fn(k, M, N, 1, flags, o, nout) if with_kn else fn(k, M, N, flags, o, nout)
        return f

    return (
        ("index_create", all_dt, True, create),
        ("search_ex", all_dt, True, ex),
        ("search_topk", all_dt, True, topk),
        ("search_range", all_dt, True, rng),
        ("plan_filter", all_dt, True, lambda dt, k, flags: L.nns_plan_filter(k, M, N, dt, flags, o, 16)),
        ("plan_topk", all_dt, False, lambda dt, k, flags: L.nns_plan_topk(k, M, N, 1, dt, o, 6)),
        ("plan_range", all_dt, False, lambda dt, k, flags: L.nns_plan_range(k, M, N, dt, o, 6)),
        ("plan_topk_mfma", (0, 1, 5), True, mfma_plan("nns_plan_topk_mfma", 17, True)),
        ("plan_range_mfma", (0, 1, 5), True, mfma_plan("nns_plan_range_mfma", 10, False)),
    )


def _answer(pkg, call, *args):
    """(status, message) of one call; "" where it sets no message (a sentinel call before it leaves a known one)."""
    L = pkg.lib
    assert L.nns_keys_topk_merge(None, None, 0, 1, None) != 0
    rc = call(*args)
    msg = L.nns_last_error().decode()
    return [int(rc), "" if rc == 0 or msg == SENTINEL else msg]


def _device_answer(pkg):
    """what a call that passes every argument check answers for device 99 on this machine"""
    L = pkg.lib
    buf = np.zeros(1024, np.float32)
    idx = np.zeros(M, np.int32)
    return _answer(pkg, lambda: L.nns_search_f32_ex(8, M, N, buf.ctypes.data, buf.ctypes.data, idx.ctypes.data, None, 1, 0,
                                                    DEVICE))


def _run_grid(pkg):
    """{"<entry>/<infix>": [answer per (k, flags) in grid order]}; an answer is [status, message] or "DEVICE"."""
    dev = _device_answer(pkg)
    assert dev[0] != 0 and dev[1]
    grid = {}
    for name, dtypes, with_flags, call in _calls(pkg):
        for dt in dtypes:
            row = []
            for k in _ks(dt):
                for flags in (FLAGS if with_flags else (0,)):
                    a = _answer(pkg, call, dt, k, flags)
                    row.append("DEVICE" if a == dev else a)
            grid[f"{name}/{INFIX[dt]}"] = row
    return grid


def record(path=GOLDEN):
    """Write the recording from the library NNS_LIB_PATH names (not collected; run on a build of the commit to record)."""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    grid = _run_grid(pkg)
    messages = sorted({a[1] for row in grid.values() for a in row if a != "DEVICE"})
    number = {s: i for i, s in enumerate(messages)}
    doc = {"library": os.path.basename(pkg.LIB_PATH), "flags": list(FLAGS), "k": list(KS), "k_bits_b1": list(KS_B1),
           "messages": messages,
           "cases": {key: ["D" if a == "DEVICE" else [a[0], number[a[1]]] for a in row] for key, row in grid.items()}}
    with open(path, "w") as f:
        f.write("{\n")
        for key in ("library", "flags", "k", "k_bits_b1"):
            f.write(f" {json.dumps(key)}: {json.dumps(doc[key])},\n")
        f.write(' "messages": [\n' + ",\n".join("  " + json.dumps(s) for s in messages) + "\n ],\n")
        f.write(' "cases": {\n' + ",\n".join(f"  {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}"
                                             for k, v in doc["cases"].items()) + "\n }\n}\n")
    total = sum(len(row) for row in grid.values())
    ndev = sum(a == "DEVICE" for row in grid.values() for a in row)
    print(f"{path}: {total} cases, {ndev} end at the device lookup, {len(messages)} distinct messages")


def _golden():
    with open(GOLDEN) as f:
        doc = json.load(f)
    assert tuple(doc["flags"]) == FLAGS and tuple(doc["k"]) == KS and tuple(doc["k_bits_b1"]) == KS_B1
    msgs = doc["messages"]
    return {key: ["DEVICE" if a == "D" else [a[0], msgs[a[1]]] for a in row] for key, row in doc["cases"].items()}


def test_the_grid_is_mostly_refusals_and_plans():
    """fewer than half of the recorded cases may end at the device lookup: the rest pin a status and its message"""
    want = _golden()
    total = sum(len(row) for row in want.values())
    ndev = sum(a == "DEVICE" for row in want.values() for a in row)
    assert total >= 3000 and 2 * ndev < total, (total, ndev)
    assert sorted(want) == sorted(f"{name}/{INFIX[dt]}" for name, dts in (
        ("index_create", range(6)), ("search_ex", range(6)), ("search_topk", range(6)), ("search_range", range(6)),
        ("plan_filter", range(6)), ("plan_topk", range(6)), ("plan_range", range(6)), ("plan_topk_mfma", (0, 1, 5)),
        ("plan_range_mfma", (0, 1, 5))) for dt in dts)


def test_every_refusal_is_the_recorded_one(pkg):
    want = _golden()
    got = _run_grid(pkg)
    assert sorted(got) == sorted(want)
    bad = []
    for key in want:
        assert len(got[key]) == len(want[key]), key
        dt = INFIX.index(key.split("/")[1])
        with_flags = len(want[key]) == len(_ks(dt)) * len(FLAGS)
        cases = [(k, f) for k in _ks(dt) for f in (FLAGS if with_flags else (0,))]
        bad += [(key, k, hex(f), g, w) for (k, f), g, w in zip(cases, got[key], want[key]) if g != w]
    assert not bad, f"{len(bad)} cases differ; the first: {bad[:5]}"


if __name__ == "__main__":
    record()
