#!/usr/bin/env python3
"""Range-search probe: Index.range_count / range_fill (K7) against the same index's top-K at kn = 1 (K6) and exact
1-NN search (NNS_PATH_EXACT), timed with HIP events over warmed back-to-back calls.  The radii are the median (over
the queries) 10th / 100th / 1000th-nearest V0 distance, taken from a top-K search, so that a query has about 10, 100
and 1000 hits.  One JSON line per (shape, radius):
    python tools/probe_range.py [--only m,n,k] [--reps N] [--out FILE]
Targets: count <= 1.1x and count + fill <= 2.3x the top-K kn = 1 time of the same shape."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402

SHAPES = [  # (m, n, k): the reference driver's largest 3-D and 16-D samples, a deep batch, one deep query
    (1024, 1 << 20, 3), (1024, 1 << 20, 16), (4096, 1 << 20, 128), (1, 1 << 20, 128),
]
HITS = (10, 100, 1000)


def _time(fn, reps):
    for _ in range(3):
        fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", help="m,n,k: one shape")
    ap.add_argument("--reps", type=int, default=0, help="timed calls per measurement (0: about 1 s of work)")
    ap.add_argument("--out", help="also append the JSON lines to this file")
    a = ap.parse_args()
    pkg = graft.load_package()
    shapes = [tuple(int(v) for v in a.only.split(","))] if a.only else SHAPES
    dev = torch.device("cuda:0")
    for m, n, k in shapes:
        q = torch.empty((m, k), dtype=torch.float32, device=dev)
        r = torch.empty((n, k), dtype=torch.float32, device=dev)
        pkg.fill_uniform(q, 1, 0)
        pkg.fill_uniform(r, 2, 0)
        ix = pkg.Index(r, path="exact")
        keys1 = torch.empty(m, dtype=torch.int64, device=dev)
        keysk = torch.empty((m, 1), dtype=torch.int64, device=dev)
        probe = _time(lambda: ix.search_topk_keys(q, 1, keys=keysk), 2)
        reps = a.reps or max(3, min(200, int(1000.0 / max(probe, 1e-3))))
        t_nn = _time(lambda: ix.search_keys(q, keys1), reps)
        t_k1 = _time(lambda: ix.search_topk_keys(q, 1, keys=keysk), reps)
        # radii: the median kn-th nearest distance (top-K of a query sample at the deepest kn)
        qs = q[:256]
        _, dk = ix.search_topk(qs, 256, return_distances=True)
        radii = {h: float(dk[:, h - 1].median()) for h in HITS if h <= 256}
        # 1000 is beyond top-K's 256: bisect the squared radius on the median range count of the same sample,
        # starting from the 100-hit radius and a bound well above (the hit count grows like radius2^(k/2))
        lo, hi = radii[100], radii[100] * (10.0 ** (2.0 / k)) * 4.0
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            if torch.diff(ix.range_count(qs, mid)).median().item() < 1000:
                lo = mid
            else:
                hi = mid
        radii[1000] = hi
        lims = torch.empty(m + 1, dtype=torch.int64, device=dev)
        for h in HITS:
            r2 = radii[h]
            ix.range_count(q, r2, lims=lims)
            total = int(lims[-1].item())
            idx = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
            dist = torch.empty(max(total, 1), dtype=torch.float32, device=dev)
            t_count = _time(lambda: ix.range_count(q, r2, lims=lims), reps)
            t_fill = _time(lambda: ix.range_fill(q, r2, lims, idx=idx, dist=dist, return_distances=True), reps)
            t_both = _time(lambda: (ix.range_count(q, r2, lims=lims),
                                    ix.range_fill(q, r2, lims, idx=idx, dist=dist, return_distances=True)), reps)
            counts = torch.diff(lims).double()
            rec = {"m": m, "n": n, "k": k, "target_hits": h, "radius2": r2, "reps": reps,
                   "hits_median": float(counts.median()), "hits_mean": round(float(counts.mean()), 2),
                   "total": total, "count_ms": round(t_count, 4), "fill_ms": round(t_fill, 4),
                   "count_fill_ms": round(t_both, 4), "topk1_ms": round(t_k1, 4), "nn1_exact_ms": round(t_nn, 4),
                   "count_over_topk1": round(t_count / t_k1, 3), "count_fill_over_topk1": round(t_both / t_k1, 3),
                   "count_target_met": t_count <= 1.1 * t_k1, "count_fill_target_met": t_both <= 2.3 * t_k1,
                   "plan": pkg.plan_range(k, m, n)}
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            del idx, dist
        ix.close()
        del q, r, keys1, keysk


if __name__ == "__main__":
    main()
