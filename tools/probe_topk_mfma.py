#!/usr/bin/env python3
"""K6m probe: the MFMA-filtered top-K search (Index(topk_mfma=True)) against K6 on the SAME index with the filtered path
switched off by an unflagged twin over the same buffers — HIP events over warmed calls, both arms of one (shape, kn) in
one process on one device, alternating: REPEATS windows per arm, each of `reps` back-to-back calls (about 0.3 s of
work), reported as min / median / max per call.  The stage split of the filtered arm comes from an NNS_PROFILE index
timed separately (bound = rerank_ms, flag = filter_ms, select = finalize_ms, K2 on the queries = prep_queries_ms);
flagged / examined from topk_info.  Keys of both arms are compared.
    python tools/probe_topk_mfma.py [--only m,n,k,kn] [--reps N] [--out profiles/topk_mfma_probe.json]
--bf16: the same on bf16 points (the uniform values rounded to bf16; cases BF16_CASES); the record goes to
profiles/topk_mfma_bf16_probe.json.
The parent starts one child per shape (never more than one process on the GPU), each under its own time limit; a child
that fails or runs out of time ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(4096, 1 << 20, 128, (1, 10, 100)), (65536, 65536, 16, (16,)), (1024, 1 << 20, 16, (10,))]   # (m, n, k, kns)
BF16_CASES = [(4096, 1 << 20, 128, (1, 10, 100)), (65536, 65536, 32, (1, 10, 100))]
REPEATS = 5
STEP_LIMIT_S = 280


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


def probe_shape(m, n, k, kns, reps_arg, bf16=False):
    import torch
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    dev = torch.device("cuda:0")
    q = torch.empty((m, k), dtype=torch.float32, device=dev)
    r = torch.empty((n, k), dtype=torch.float32, device=dev)
    pkg.fill_uniform(q, 1, 0)
    pkg.fill_uniform(r, 2, 0)
    if bf16:
        q, r = q.to(torch.bfloat16), r.to(torch.bfloat16)
    k6 = pkg.Index(r, path="exact")
    fx = pkg.Index(r, path="exact", topk_mfma=True)
    pf = pkg.Index(r, path="exact", topk_mfma=True, profile=True)
    out = []
    for kn in kns:
        keys6 = torch.empty((m, kn), dtype=torch.int64, device=dev)
        keysm = torch.empty((m, kn), dtype=torch.int64, device=dev)
        arms = {"k6": lambda: k6.search_topk_keys(q, kn, keys=keys6), "k6m": lambda: fx.search_topk_keys(q, kn, keys=keysm)}
        reps = {}
        for name, fn in arms.items():
            fn()
            one = _window(torch, fn, 1)                  # (warmed by the call above)
            reps[name] = reps_arg or max(2, min(200, int(300.0 / max(one, 1e-3))))
        info = fx.topk_info()
        same = bool(torch.equal(keys6, keysm))
        times = {name: [] for name in arms}
        for _ in range(REPEATS):                         # alternate the arms
            for name, fn in arms.items():
                times[name].append(_window(torch, fn, reps[name]))
        pf.search_topk_keys(q, kn, keys=keysm)
        pf.stats()
        _window(torch, lambda: pf.search_topk_keys(q, kn, keys=keysm), min(reps["k6m"], 30))
        st = pf.stats()                                  # the averages of the calls just timed
        t6, tm = _mmm(times["k6"]), _mmm(times["k6m"])
        # the gain counts only beyond both arms' run-to-run spread
        beats = t6["min"] - tm["max"] > 0 and (t6["median"] - tm["median"]) > (t6["max"] - t6["min"]) + (tm["max"] - tm["min"])
        out.append({"m": m, "n": n, "k": k, "bf16": bf16, "kn": kn, "reps": reps, "repeats": REPEATS, "keys_equal_k6": same,
                    "k6_ms": t6, "k6m_ms": tm, "k6_over_k6m": round(t6["median"] / tm["median"], 2),
                    "beats_k6_beyond_spread": bool(beats), "topk_info": info,
                    "flagged_over_examined": round(info["flagged"] / info["examined"], 5) if info["examined"] else None,
                    "stages_ms": {"bound": round(st["rerank_ms"], 4), "prep_queries": round(st["prep_queries_ms"], 4),
                                  "flag": round(st["filter_ms"], 4), "select": round(st["finalize_ms"], 4),
                                  "total": round(st["total_ms"], 4)},
                    "plan": pkg.plan_topk_mfma(k, m, n, kn, bf16=bf16)})
    for ix in (k6, fx, pf):
        ix.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", help="m,n,k,kn: one shape at one kn")
    ap.add_argument("--reps", type=int, default=0, help="calls per timed window (0: about 0.3 s of work)")
    ap.add_argument("--bf16", action="store_true", help="bf16 points (32 <= k <= 256)")
    ap.add_argument("--out", help="default: profiles/topk_mfma_probe.json, with --bf16 profiles/topk_mfma_bf16_probe.json")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        m, n, k, *kns = (int(v) for v in a.child.split(","))
        print("RESULT " + json.dumps(probe_shape(m, n, k, kns, a.reps, a.bf16)), flush=True)
        return 0
    out_path = a.out or os.path.join(ROOT, "profiles", "topk_mfma_bf16_probe.json" if a.bf16 else "topk_mfma_probe.json")
    cases = BF16_CASES if a.bf16 else CASES
    if a.only:
        m, n, k, kn = (int(v) for v in a.only.split(","))
        cases = [(m, n, k, (kn,))]
    records = []
    for m, n, k, kns in cases:   # one child at a time; the first failure ends the run
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child",
               ",".join(str(v) for v in (m, n, k) + tuple(kns)), "--reps", str(a.reps)] + (["--bf16"] if a.bf16 else [])
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print(f"shape {m} x {n} x {k}: child ended with status {p.returncode}; stopping", file=sys.stderr)
            return 1
        for line in p.stdout.splitlines():
            if line.startswith("RESULT "):
                recs = json.loads(line[len("RESULT "):])
                records += recs
                for rec in recs:
                    print(json.dumps(rec), flush=True)
    with open(out_path, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
