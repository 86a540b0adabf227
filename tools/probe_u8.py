#!/usr/bin/env python3
"""uint8 probe.  One process per shape on one device, the arms of a comparison alternating, ROUNDS rounds, every pair of arms
asserted to return equal keys / lims / indices, medians and spread (min, max) recorded:
  1-NN   a uint8 index next to an int8 index on the values - 128: the same filter kernel (filter_i8_kernel) on the same
         image, so the difference is K2's (the bias) and K5's (the uint8 re-rank) only.  Stage times from NNS_PROFILE.
  top-K  a uint8 index with NNS_TOPK_MFMA (K6m on range_flag_u8_kernel) next to one without (K6), kn = 1 / 10 / 100.
  range  count + fill at about 100 hits per query, with NNS_RANGE_MFMA (K7m) next to without (K7).
  flag   the flag pass alone: filter_ms of the flagged index's count pass, next to the time recorded for the bf16 flag
         pass at the same shape (README; profiles/range_mfma_bf16_probe.json).
    python tools/probe_u8.py [--only m,n,k] [--out profiles/u8_probe.json]
The parent starts one child per shape (never more than one process on the GPU), each under its own time limit; a child
that fails or runs out of time ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(4096, 1 << 20, 128), (65536, 65536, 32)]   # (m, n, k)
ROUNDS = 3
STEP_LIMIT_S = 400
STAGES = ("prep_queries_ms", "filter_ms", "finalize_ms", "rerank_ms", "total_ms")
BF16_FLAG_PASS_MS = {(4096, 1 << 20, 128): 0.95, (65536, 65536, 32): 0.89}   # recorded for range_flag16_kernel


def _window(torch, fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def _mmm(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)}


def _alternate(torch, run, reps):
    """{arm: [per-call ms of each round]} of the arms of `run`, alternating"""
    for fn in run.values():
        fn()                                             # warm: code objects, workspaces
    wall = {name: [] for name in run}
    for _ in range(ROUNDS):
        for name, fn in run.items():
            wall[name].append(_window(torch, fn, reps))
    return wall


def _pair(wall, fast, slow):
    """the record of two arms: min / median / max each, the ratio of the medians, and whether the fast arm's gain exceeds
    the two arms' min-to-max ranges together"""
    f, s = _mmm(wall[fast]), _mmm(wall[slow])
    spread = (f["max"] - f["min"]) + (s["max"] - s["min"])
    return {fast + "_ms": f, slow + "_ms": s, "ratio": round(s["median"] / f["median"], 3),
            "faster_beyond_spread": bool(s["median"] - f["median"] > spread)}


def probe_shape(m, n, k):
    import torch
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000 + k)
    q = torch.randint(0, 256, (m, k), dtype=torch.uint8, device=dev, generator=gen)
    r = torch.randint(0, 256, (n, k), dtype=torch.uint8, device=dev, generator=gen)
    q8 = (q.to(torch.int16) - 128).to(torch.int8)
    r8 = (r.to(torch.int16) - 128).to(torch.int8)
    rec = {"m": m, "n": n, "k": k, "rounds": ROUNDS}

    # ---- 1-NN: uint8 against int8 on the values - 128 ----
    arms = {"u8": pkg.Index(r, points="u8", profile=True), "i8": pkg.Index(r8, profile=True)}
    qs = {"u8": q, "i8": q8}
    keys = {name: torch.empty(m, dtype=torch.int64, device=dev) for name in arms}
    run = {name: (lambda name=name: arms[name].search_keys(qs[name], keys=keys[name])) for name in arms}
    for name, fn in run.items():
        fn()
        arms[name].stats()                               # (start the averages afresh)
    reps = 30
    wall = {name: [] for name in arms}
    stages = {name: {s: [] for s in STAGES} for name in arms}
    for _ in range(ROUNDS):
        for name, fn in run.items():
            wall[name].append(_window(torch, fn, reps))
            st = arms[name].stats()
            for s in STAGES:
                stages[name][s].append(st[s])
    torch.cuda.synchronize()
    assert torch.equal(keys["u8"], keys["i8"]), "the uint8 and the int8 index returned different keys"
    one = _pair(wall, "i8", "u8")
    one.update({"reps": reps, "keys_equal": True,
                "u8_stages_ms": {s: _mmm(stages["u8"][s]) for s in STAGES},
                "i8_stages_ms": {s: _mmm(stages["i8"][s]) for s in STAGES},
                "filter_form": arms["u8"].stats()["filter_form"]})
    rec["nn1"] = one
    for ix in arms.values():
        ix.close()
    del r8, q8

    # ---- top-K and range search: the flag pass against the exact scans ----
    flagged = pkg.Index(r, points="u8", range_mfma=True, topk_mfma=True, profile=True)
    plain = pkg.Index(r, points="u8")
    rec["topk"] = {}
    for kn in (1, 10, 100):
        out = {name: torch.empty((m, kn), dtype=torch.int64, device=dev) for name in ("k6m", "k6")}
        run = {"k6m": lambda: flagged.search_topk_keys(q, kn, keys=out["k6m"]),
               "k6": lambda: plain.search_topk_keys(q, kn, keys=out["k6"])}
        wall = _alternate(torch, run, 2)
        torch.cuda.synchronize()
        assert torch.equal(out["k6m"], out["k6"]), f"K6m and K6 returned different keys at kn = {kn}"
        info = flagged.topk_info()
        assert info["path"] == 2, info
        one = _pair(wall, "k6m", "k6")
        one.update({"keys_equal": True, "flagged": info["flagged"], "examined": info["examined"], "filled": info["filled"]})
        rec["topk"][str(kn)] = one
    # about 100 hits per query: the median 100th distance of a sample of queries
    sample = plain.search_topk_keys(q[:256].contiguous(), 100)
    radius2 = float((sample[:, 99] >> 32).to(torch.int32).view(torch.float32).median().item())
    res = {}
    run = {"k7m": lambda: res.__setitem__("k7m", flagged.search_range(q, radius2)),
           "k7": lambda: res.__setitem__("k7", plain.search_range(q, radius2))}
    wall = _alternate(torch, run, 1)
    torch.cuda.synchronize()
    for a, b in zip(res["k7m"], res["k7"]):
        assert torch.equal(a, b), "K7m and K7 returned different lims / indices"
    info = flagged.range_info()
    assert info["path"] == 2, info
    one = _pair(wall, "k7m", "k7")
    one.update({"radius2": radius2, "hits_per_query": round(info["hits"] / m, 2), "results_equal": True,
                "flagged": info["flagged"], "examined": info["examined"]})
    rec["range"] = one

    # ---- the flag pass alone: the count pass's stages ----
    flagged.stats()
    fl = {s: [] for s in STAGES}
    for _ in range(ROUNDS):
        for _ in range(5):
            flagged.range_count(q, radius2)
        st = flagged.stats()
        for s in STAGES:
            fl[s].append(st[s])
    rec["flag_pass"] = {"count_stages_ms": {s: _mmm(fl[s]) for s in STAGES},
                        "flag_pass_ms": _mmm(fl["filter_ms"]),
                        "bf16_flag_pass_ms_recorded": BF16_FLAG_PASS_MS.get((m, n, k))}
    flagged.close()
    plain.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", help="m,n,k: one shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "u8_probe.json"))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        m, n, k = (int(v) for v in a.child.split(","))
        print("RESULT " + json.dumps(probe_shape(m, n, k)), flush=True)
        return 0
    cases = [tuple(int(v) for v in a.only.split(","))] if a.only else CASES
    records = []
    for m, n, k in cases:   # one child at a time; the first failure ends the run
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", f"{m},{n},{k}"]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print(f"shape {m} x {n} x {k}: child ended with status {p.returncode}; stopping", file=sys.stderr)
            return 1
        for line in p.stdout.splitlines():
            if line.startswith("RESULT "):
                rec = json.loads(line[len("RESULT "):])
                records.append(rec)
                print(json.dumps(rec), flush=True)
    with open(a.out, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
