#!/usr/bin/env python3
"""int8 probe: the 1-NN search of an int8 index (v_mfma_i32_16x16x64_i8 filter, exact integer scores) next to a bf16 index
of the same build on the SAME integer values (uniform over -128 .. 127: every int8 value is exact in bf16, and so is
-2 v) — both NNS_PROFILE indexes in one process on one device, alternating, ROUNDS rounds per shape.  A round is one
window of `reps` back-to-back searches per arm (about 0.3 s of work) timed with HIP events, then the arm's
nns_index_stats: the stage averages over the searches just timed (K2 on the queries, filter, K5, re-rank, total) and the
counters of the last one.  Reported per arm as min / median / max over the rounds.  The two arms answer the same
question: the probe asserts that they return equal keys.
    python tools/probe_i8.py [--only m,n,k] [--reps N] [--out profiles/i8_probe.json]
The parent starts one child per shape (never more than one process on the GPU), each under its own time limit; a child
that fails or runs out of time ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(4096, 1 << 20, 128), (4096, 1 << 20, 256), (65536, 65536, 32)]   # (m, n, k)
ROUNDS = 3
STEP_LIMIT_S = 240
STAGES = ("prep_queries_ms", "filter_ms", "finalize_ms", "rerank_ms", "total_ms")


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


def probe_shape(m, n, k, reps_arg):
    import torch
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000 + k)
    q = torch.randint(-128, 128, (m, k), dtype=torch.int8, device=dev, generator=gen)
    r = torch.randint(-128, 128, (n, k), dtype=torch.int8, device=dev, generator=gen)
    pts = {"i8": (q, r), "bf16": (q.to(torch.bfloat16), r.to(torch.bfloat16))}
    assert torch.equal(pts["bf16"][1][:4096].to(torch.int8), r[:4096])       # (the same values)
    del q, r
    arms, keys, reps = {}, {}, {}
    for name, (qq, rr) in pts.items():
        arms[name] = pkg.Index(rr, profile=True)
        keys[name] = torch.empty(m, dtype=torch.int64, device=dev)
    run = {name: (lambda name=name: arms[name].search_keys(pts[name][0], keys=keys[name])) for name in arms}
    build = {}
    for name, fn in run.items():
        build[name] = round(arms[name].stats()["prep_refs_ms"], 4)      # K2 on the refs, from the index build
        fn()
        one = _window(torch, fn, 1)                      # (warmed by the call above)
        reps[name] = reps_arg or max(2, min(30, int(300.0 / max(one, 1e-3))))   # (at most the 32 event sets of an index)
        arms[name].stats()                               # (start the averages afresh)
    wall = {name: [] for name in arms}
    stages = {name: {s: [] for s in STAGES} for name in arms}
    last = {}
    for _ in range(ROUNDS):                              # alternate the arms
        for name, fn in run.items():
            wall[name].append(_window(torch, fn, reps[name]))
            st = arms[name].stats()
            for s in STAGES:
                stages[name][s].append(st[s])
            last[name] = st
    rec = {"m": m, "n": n, "k": k, "rounds": ROUNDS, "reps": reps}
    for name in arms:
        st = last[name]
        rec[name] = {"per_search_ms": _mmm(wall[name]), "stages_ms": {s: _mmm(stages[name][s]) for s in STAGES},
                     "prep_refs_ms": build[name], "path": st["path"], "k_tile": st["k_tile"], "splits": st["splits"],
                     "filter_form": st["filter_form"], "ambiguous": st["ambiguous"], "multi_candidate": st["multi_candidate"],
                     "nonfinite": st["nonfinite"]}
    torch.cuda.synchronize()
    rec["keys_equal"] = bool(torch.equal(keys["i8"], keys["bf16"]))
    assert rec["keys_equal"], "the int8 and the bf16 index returned different keys"
    f, b = rec["i8"], rec["bf16"]
    rec["i8_over_bf16"] = {"per_search": round(f["per_search_ms"]["median"] / b["per_search_ms"]["median"], 4),
                            "filter": round(f["stages_ms"]["filter_ms"]["median"] / b["stages_ms"]["filter_ms"]["median"], 4)}
    # "equal within the rounds' spread": the medians differ by no more than the two arms' min-to-max ranges together
    spread = (f["per_search_ms"]["max"] - f["per_search_ms"]["min"]) + (b["per_search_ms"]["max"] - b["per_search_ms"]["min"])
    rec["equal_within_spread"] = bool(abs(f["per_search_ms"]["median"] - b["per_search_ms"]["median"]) <= spread)
    for ix in arms.values():
        ix.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", help="m,n,k: one shape")
    ap.add_argument("--reps", type=int, default=0, help="searches per timed window (0: about 0.3 s of work, at most 30)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "i8_probe.json"))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        m, n, k = (int(v) for v in a.child.split(","))
        print("RESULT " + json.dumps(probe_shape(m, n, k, a.reps)), flush=True)
        return 0
    cases = [tuple(int(v) for v in a.only.split(","))] if a.only else CASES
    records = []
    for m, n, k in cases:   # one child at a time; the first failure ends the run
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child",
               f"{m},{n},{k}", "--reps", str(a.reps)]
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
