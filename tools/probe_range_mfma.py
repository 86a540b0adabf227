#!/usr/bin/env python3
"""K7m probe: the MFMA-filtered range search (Index(range_mfma=True)) against K7 on an unflagged index over the same
buffers, and its flag pass against the eager split 1-NN filter of the same shape — HIP events over warmed back-to-back
calls, everything of one shape in one process on one device.  Radii: the median (over a query sample) 10th / 100th /
1000th-nearest V0 distance.  Per (shape, radius): filtered count, fill and their sum, the flag pass alone (NNS_PROFILE's
filter_ms of the count), range_info, K7 count + fill, and the 1-NN filter_ms of a filter_split_eager index (nn1_filter
names the filter compared with).
    python tools/probe_range_mfma.py [--only m,n,k] [--reps N] [--out profiles/range_mfma_probe.json]
--bf16: the same on bf16 points (the uniform values rounded to bf16; shapes BF16_SHAPES, 100 hits per query); the 1-NN
filter it is held against is then the bf16 one, and the record goes to profiles/range_mfma_bf16_probe.json.
The parent starts one child per shape (never more than one process on the GPU), each under its own time limit; a child
that fails or runs out of time ends the run."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(4096, 1 << 20, 128), (1024, 1 << 20, 16), (65536, 65536, 64)]   # (m, n, k)
BF16_SHAPES = [(4096, 1 << 20, 128), (65536, 65536, 32)]
HITS = (10, 100, 1000)
STEP_LIMIT_S = 240


def _time(torch, fn, reps):
    for _ in range(2):
        fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def probe_shape(m, n, k, reps_arg, bf16=False):
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
    hits = (100,) if bf16 else HITS
    k7 = pkg.Index(r, path="exact")
    fx = pkg.Index(r, range_mfma=True, profile=True)
    nn = pkg.Index(r, path="mfma", profile=True) if bf16 else pkg.Index(r, path="mfma", filter_split_eager=True, profile=True)
    nn_name = "bf16 16x16x32" if bf16 else "eager split"
    # radii from a query sample: top-K up to 256, the 1000-hit radius by bisection on K7's count
    qs = q[:256]
    _, dk = k7.search_topk(qs, 256, return_distances=True)
    radii = {h: float(dk[:, h - 1].median()) for h in HITS if h <= 256}
    lo, hi = radii[100], radii[100] * (10.0 ** (2.0 / k)) * 4.0
    for _ in range(30):
        mid = 0.5 * (lo + hi)
        if torch.diff(k7.range_count(qs, mid)).median().item() < 1000:
            lo = mid
        else:
            hi = mid
    radii[1000] = hi
    keys = torch.empty(m, dtype=torch.int64, device=dev)
    probe = _time(torch, lambda: nn.search_keys(q, keys), 1)
    nn.stats()
    reps_nn = reps_arg or max(3, min(50, int(500.0 / max(probe, 1e-3))))
    _time(torch, lambda: nn.search_keys(q, keys), reps_nn)
    nn_filter_ms = nn.stats()["filter_ms"]
    out = []
    lims = torch.empty(m + 1, dtype=torch.int64, device=dev)
    lims7 = torch.empty(m + 1, dtype=torch.int64, device=dev)
    for h in hits:
        r2 = radii[h]
        fx.range_count(q, r2, lims=lims)
        info = fx.range_info()
        total = int(lims[-1].item())
        idx = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        dist = torch.empty(max(total, 1), dtype=torch.float32, device=dev)
        fill = lambda ix, lm: ix.range_fill(q, r2, lm, idx=idx, dist=dist, return_distances=True)  # noqa: E731
        one = _time(torch, lambda: (k7.range_count(q, r2, lims=lims7), fill(k7, lims7)), 1)
        reps = reps_arg or max(3, min(50, int(500.0 / max(one, 1e-3))))
        t_k7 = _time(torch, lambda: (k7.range_count(q, r2, lims=lims7), fill(k7, lims7)), reps)
        same = bool(torch.equal(lims, lims7))
        fx.stats()
        t_count = _time(torch, lambda: fx.range_count(q, r2, lims=lims), reps)
        st = fx.stats()                                  # the averages of the counts just timed
        t_fill = _time(torch, lambda: fill(fx, lims), reps)
        t_both = _time(torch, lambda: (fx.range_count(q, r2, lims=lims), fill(fx, lims)), reps)
        fx.stats()
        out.append({"m": m, "n": n, "k": k, "bf16": bf16, "target_hits": h, "radius2": r2, "reps": reps, "total": total,
                    "hits_mean": round(total / m, 2), "range_info": info, "lims_equal_k7": same,
                    "count_ms": round(t_count, 4), "fill_ms": round(t_fill, 4), "count_fill_ms": round(t_both, 4),
                    "flag_pass_ms": round(st["filter_ms"], 4), "prep_queries_ms": round(st["prep_queries_ms"], 4),
                    "eval_count_ms": round(st["finalize_ms"], 4),
                    "k7_count_fill_ms": round(t_k7, 4), "k7_over_filtered": round(t_k7 / t_both, 2),
                    "nn1_filter": nn_name, "nn1_filter_ms": round(nn_filter_ms, 4),
                    "flag_over_nn1_filter": round(st["filter_ms"] / nn_filter_ms, 3) if nn_filter_ms > 0 else None,
                    "plan": pkg.plan_range_mfma(k, m, n, bf16=bf16)})
        del idx, dist
    for ix in (k7, fx, nn):
        ix.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", help="m,n,k: one shape")
    ap.add_argument("--reps", type=int, default=0, help="timed calls per measurement (0: about 0.5 s of work)")
    ap.add_argument("--bf16", action="store_true", help="bf16 points (32 <= k <= 256)")
    ap.add_argument("--out", help="default: profiles/range_mfma_probe.json, with --bf16 profiles/range_mfma_bf16_probe.json")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        m, n, k = (int(v) for v in a.child.split(","))
        print("RESULT " + json.dumps(probe_shape(m, n, k, a.reps, a.bf16)), flush=True)
        return 0
    out_path = a.out or os.path.join(ROOT, "profiles", "range_mfma_bf16_probe.json" if a.bf16 else "range_mfma_probe.json")
    shapes = [tuple(int(v) for v in a.only.split(","))] if a.only else (BF16_SHAPES if a.bf16 else SHAPES)
    records = []
    for m, n, k in shapes:   # one child at a time; the first failure ends the run
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", f"{m},{n},{k}",
               "--reps", str(a.reps)] + (["--bf16"] if a.bf16 else [])
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
