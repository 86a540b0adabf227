#!/usr/bin/env python3
"""A/B of two BUILDS of the library on bf16 points: arm a = a library without the bf16 flag pass (the parent commit's,
tools/build_variant.sh parent at that commit: its K7 / K6 answer), arm b = this tree's library (K7m / K6m), same data,
same device, alternating, one process per (arm, round) through NNS_LIB_PATH, ROUNDS rounds.  Per shape: range search
(count + fill) at about 100+ hits per query and top-K at kn = 1 / 10 / 100, HIP events over warmed back-to-back calls
(about 0.3 s of work each); totals and key sums of both arms compared.
    python tools/ab_flag_bf16.py A.so [B.so] [--out profiles/flag_bf16_ab.jsonl]
A child that fails or runs out of time ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(4096, 1 << 20, 128), (65536, 65536, 32)]
KNS = (1, 10, 100)
ROUNDS = 3


def _window(torch, fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def child(m, n, k, arm):
    import torch
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    dev = torch.device("cuda:0")
    q = torch.empty((m, k), dtype=torch.float32, device=dev)
    r = torch.empty((n, k), dtype=torch.float32, device=dev)
    pkg.fill_uniform(q, 1, 0)
    pkg.fill_uniform(r, 2, 0)
    q, r = q.to(torch.bfloat16), r.to(torch.bfloat16)
    new = arm == "b"                                     # (arm a's library rejects the flags for bf16 points)
    ex = pkg.Index(r, path="exact")
    _, dk = ex.search_topk(q[:256].contiguous(), 100, return_distances=True)
    r2 = float(dk[:, 99].median())
    ix = pkg.Index(r, path="exact", range_mfma=True, topk_mfma=True) if new else ex
    rec = {"arm": arm, "lib": os.path.basename(pkg.LIB_PATH), "m": m, "n": n, "k": k, "radius2": r2}
    lims = torch.empty(m + 1, dtype=torch.int64, device=dev)
    ix.range_count(q, r2, lims=lims)
    total = int(lims[-1].item())
    idx = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    dist = torch.empty(max(total, 1), dtype=torch.float32, device=dev)
    fn = lambda: (ix.range_count(q, r2, lims=lims), ix.range_fill(q, r2, lims, total=total, idx=idx, dist=dist, return_distances=True))  # noqa: E731
    fn()
    one = _window(torch, fn, 1)
    reps = max(2, min(100, int(300.0 / max(one, 1e-3))))
    rec["range_ms"] = round(_window(torch, fn, reps), 4)
    rec["range_total"] = total
    rec["range_sha"] = int(idx[:total].to(torch.int64).sum().item()) ^ int(dist[:total].view(torch.int32).to(torch.int64).sum().item())
    rec["range_path"] = ix.range_info()["path"]
    for kn in KNS:
        keys = torch.empty((m, kn), dtype=torch.int64, device=dev)
        f2 = lambda: ix.search_topk_keys(q, kn, keys=keys)  # noqa: E731
        f2()
        one = _window(torch, f2, 1)
        reps = max(2, min(100, int(300.0 / max(one, 1e-3))))
        rec[f"topk{kn}_ms"] = round(_window(torch, f2, reps), 4)
        rec[f"topk{kn}_sum"] = int((keys & 0xFFFFFFFF).sum().item())
        rec[f"topk{kn}_path"] = ix.topk_info()["path"]
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        m, n, k = (int(v) for v in sys.argv[2].split(","))
        child(m, n, k, sys.argv[3])
        return 0
    ap = argparse.ArgumentParser()
    ap.add_argument("a", help="arm a: a library built from the commit before the bf16 flag pass")
    ap.add_argument("b", nargs="?", default=os.path.join(ROOT, "nns-cuda_amd", "libnns_mi355x.so"), help="arm b (default: this tree's)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flag_bf16_ab.jsonl"))
    args = ap.parse_args()
    libs = {"a": os.path.abspath(args.a), "b": os.path.abspath(args.b)}
    out = open(args.out, "w")
    for m, n, k in SHAPES:
        recs = {"a": [], "b": []}
        for _ in range(ROUNDS):
            for arm in ("a", "b"):
                env = dict(os.environ, NNS_LIB_PATH=libs[arm])
                p = subprocess.run(["timeout", "-k", "10", "150", sys.executable, os.path.abspath(__file__), "--child", f"{m},{n},{k}", arm],
                                   stdout=subprocess.PIPE, text=True, env=env)
                if p.returncode != 0:
                    print(f"child {arm} {m}x{n}x{k} ended with {p.returncode}; stopping", file=sys.stderr)
                    return 1
                for line in p.stdout.splitlines():
                    if line.startswith("RESULT "):
                        recs[arm].append(json.loads(line[7:]))
        summary = {"probe": "tools/ab_flag_bf16.py", "m": m, "n": n, "k": k,
                   "a": os.path.basename(libs["a"]) + " (K7 / K6)", "b": os.path.basename(libs["b"]) + " (K7m / K6m)",
                   "rounds": ROUNDS, "radius2": recs["a"][0]["radius2"]}
        for key in ["range_ms"] + [f"topk{kn}_ms" for kn in KNS]:
            va, vb = [x[key] for x in recs["a"]], [x[key] for x in recs["b"]]
            summary[key] = {"a": va, "b": vb, "a_over_b_median": round(statistics.median(va) / statistics.median(vb), 2)}
        summary["range_total"] = [recs["a"][0]["range_total"], recs["b"][0]["range_total"]]
        summary["results_equal"] = all(recs["a"][0][f] == recs["b"][0][f] for f in ["range_total", "range_sha"] + [f"topk{kn}_sum" for kn in KNS])
        summary["paths_b"] = {f: recs["b"][0][f] for f in ["range_path"] + [f"topk{kn}_path" for kn in KNS]}
        line = json.dumps(summary)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
