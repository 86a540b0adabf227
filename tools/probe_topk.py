#!/usr/bin/env python3
"""Top-K probe: Index.search_topk (K6 scan + split merge) against the same index's exact 1-NN search
(NNS_PATH_EXACT), timed with HIP events over warmed back-to-back calls.  One JSON line per shape:
    python tools/probe_topk.py [--only m,n,k,kn] [--reps N] [--out FILE]
The refs stream rate counts n * k * 4 bytes per call (the bound of the m = 1 shape)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402

SHAPES = [  # (m, n, k, kn)
    (4096, 1 << 20, 128, 1), (4096, 1 << 20, 128, 10), (4096, 1 << 20, 128, 100),
    (1024, 1 << 20, 3, 10),
    (1, 1 << 20, 128, 10),
    (65536, 65536, 16, 16),
]


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
    ap.add_argument("--only", help="m,n,k,kn: one shape")
    ap.add_argument("--reps", type=int, default=0, help="timed calls per shape (0: about 1 s of work)")
    ap.add_argument("--out", help="also append the JSON lines to this file")
    a = ap.parse_args()
    pkg = graft.load_package()
    shapes = [tuple(int(v) for v in a.only.split(","))] if a.only else SHAPES
    dev = torch.device("cuda:0")
    for m, n, k, kn in shapes:
        q = torch.empty((m, k), dtype=torch.float32, device=dev)
        r = torch.empty((n, k), dtype=torch.float32, device=dev)
        pkg.fill_uniform(q, 1, 0)
        pkg.fill_uniform(r, 2, 0)
        ix = pkg.Index(r, path="exact")
        keys1 = torch.empty(m, dtype=torch.int64, device=dev)
        keysk = torch.empty((m, kn), dtype=torch.int64, device=dev)
        probe = _time(lambda: ix.search_keys(q, keys1), 2)
        reps = a.reps or max(3, min(200, int(1000.0 / max(probe, 1e-3))))
        t1 = _time(lambda: ix.search_keys(q, keys1), reps)
        tk = _time(lambda: ix.search_topk_keys(q, kn, keys=keysk), reps)
        torch.cuda.synchronize()
        same = bool(torch.equal(keysk[:, 0], keys1))
        plan = pkg.plan_topk(k, m, n, kn)
        rec = {"m": m, "n": n, "k": k, "kn": kn, "reps": reps, "nn1_exact_ms": round(t1, 4), "topk_ms": round(tk, 4),
               "ratio": round(tk / t1, 3), "topk_gpairs_per_s": round(m * n / tk / 1e6, 2),
               "topk_ref_stream_tb_per_s": round(n * k * 4 / tk / 1e9, 3), "first_column_equals_1nn": same,
               "plan": plan}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        ix.close()
        del q, r, keys1, keysk


if __name__ == "__main__":
    main()
