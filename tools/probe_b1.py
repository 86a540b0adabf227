#!/usr/bin/env python3
"""Binary-point probe: a b1 index (packed bits, the Hamming scans of K1b / K6 / K7) next to an int8 index of the same
build on the SAME bits unpacked to 0 / 1 values — the route such data took before — both in one process on one device,
alternating, ROUNDS rounds per shape.  Three runs per arm and round, each one window of `reps` back-to-back passes timed
with HIP events: the 1-NN search, top-K at kn = 10, and count + fill of a range search at about 100 hits per query (the
radius is the median kn-th Hamming distance of a sample: 256 queries against the first 65536 refs, kn scaled to the
sample).  Reported per arm and run as min / median / max over the rounds, in pairs per second, and for the b1 arm as
the fraction of the VALU issue bound of 2 kw instructions per 64 pairs (kw = k / 32; one wave-instruction per SIMD and
4 cycles at the device's clock).  The two arms answer the same question: the probe asserts equal keys, lims and indices.
    python tools/probe_b1.py [--only m,n,k] [--reps N] [--out profiles/b1_probe.json]
The parent starts one child per shape (never more than one process on the GPU), each under its own time limit; a child
that fails or runs out of time ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(4096, 1 << 20, 256), (4096, 1 << 20, 1024), (65536, 65536, 256)]   # (m, n, k bits)
ROUNDS = 3
KN = 10
HITS = 100
STEP_LIMIT_S = 280
RUNS = ("nn", "topk", "range")


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


def _unpack(torch, packed):
    """uint8 [n][kb] packed bits -> int8 [n][8 kb] of 0 / 1 (bit t of a point = bit t % 8 of byte t / 8)"""
    out = torch.empty((packed.shape[0], packed.shape[1] * 8), dtype=torch.int8, device=packed.device)
    sh = torch.arange(8, dtype=torch.uint8, device=packed.device)
    step = max(1, (1 << 27) // (packed.shape[1] * 8))
    for i0 in range(0, packed.shape[0], step):
        p = packed[i0:i0 + step]
        out[i0:i0 + step] = ((p.unsqueeze(-1) >> sh) & 1).reshape(p.shape[0], -1).to(torch.int8)
    return out


def probe_shape(m, n, k, reps_arg):
    import torch
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(2000 + k)
    qb = torch.randint(0, 256, (m, k // 8), dtype=torch.uint8, device=dev, generator=gen)
    rb = torch.randint(0, 256, (n, k // 8), dtype=torch.uint8, device=dev, generator=gen)
    pts = {"b1": (qb, rb), "i8": (_unpack(torch, qb), _unpack(torch, rb))}
    arms = {name: pkg.Index(rr) for name, (_, rr) in pts.items()}
    # the radius: the median kn-th distance of a sample, kn scaled to the sample's share of the refs
    ns, ms = min(n, 65536), min(m, 256)
    kns = max(1, min(256, round(HITS * ns / n)))
    sample = pkg.Index(rb[:ns])
    sd = sample.search_topk(qb[:ms], kns, return_distances=True)[1][:, -1]
    radius2 = float(sd.median().item())
    sample.close()
    out = {}
    for name, ix in arms.items():
        qq = pts[name][0]
        lims = ix.range_count(qq, radius2)
        total = int(lims[-1].item())
        out[name] = {"keys": torch.empty(m, dtype=torch.int64, device=dev),
                     "tk": torch.empty((m, KN), dtype=torch.int64, device=dev), "lims": lims,
                     "idx": torch.empty(total, dtype=torch.int32, device=dev), "total": total}

    def runs_of(name):
        ix, qq, o = arms[name], pts[name][0], out[name]

        def rng():
            ix.range_count(qq, radius2, lims=o["lims"])
            ix.range_fill(qq, radius2, o["lims"], total=o["total"], idx=o["idx"])
        return {"nn": lambda: ix.search_keys(qq, keys=o["keys"]), "topk": lambda: ix.search_topk_keys(qq, KN, keys=o["tk"]),
                "range": rng}

    run = {name: runs_of(name) for name in arms}
    reps = {name: {} for name in arms}
    for name in arms:
        for what, fn in run[name].items():
            fn()
            one = _window(torch, fn, 1)                     # (warmed by the call above)
            reps[name][what] = reps_arg or max(1, min(20, int(300.0 / max(one, 1e-3))))
    wall = {name: {what: [] for what in RUNS} for name in arms}
    for _ in range(ROUNDS):                                 # alternate the arms
        for name in arms:
            for what in RUNS:
                wall[name][what].append(_window(torch, run[name][what], reps[name][what]))
    torch.cuda.synchronize()
    props = torch.cuda.get_device_properties(0)
    clock_hz = float(getattr(props, "clock_rate", 0)) * 1e3 or 2.4e9     # (kHz; MI355X: 2.4 GHz peak)
    simds = props.multi_processor_count * 4
    pairs = float(m) * float(n)
    kw = k // 32
    bound_ms = {"nn": pairs / 64 * 2 * kw * 4 / (simds * clock_hz) * 1e3}
    bound_ms["topk"] = bound_ms["nn"]
    bound_ms["range"] = 2 * bound_ms["nn"]                  # count and fill each scan every pair
    rec = {"m": m, "n": n, "k_bits": k, "kw": kw, "rounds": ROUNDS, "kn": KN, "radius2": radius2,
           "hits_per_query": round(out["b1"]["total"] / m, 2), "reps": reps, "clock_hz": clock_hz, "simds": simds,
           "valu_bound_ms": {w: round(v, 4) for w, v in bound_ms.items()}}
    for name in arms:
        st = arms[name].stats()
        rec[name] = {"path": st["path"], "filter_form": st["filter_form"]}
        for what in RUNS:
            t = _mmm(wall[name][what])
            rec[name][what] = {"ms": t, "pairs_per_s": round(pairs * (2 if what == "range" else 1) / (t["median"] * 1e-3), 1),
                               "spread": round((t["max"] - t["min"]) / t["median"], 4)}
    rec["keys_equal"] = bool(torch.equal(out["b1"]["keys"], out["i8"]["keys"]) and torch.equal(out["b1"]["tk"], out["i8"]["tk"])
                             and torch.equal(out["b1"]["lims"], out["i8"]["lims"]) and torch.equal(out["b1"]["idx"], out["i8"]["idx"]))
    assert rec["keys_equal"], "the b1 and the int8 index returned different keys, lims or indices"
    rec["b1_valu_bound_fraction"] = {w: round(bound_ms[w] / rec["b1"][w]["ms"]["median"], 4) for w in RUNS}
    rec["i8_over_b1"] = {w: round(rec["i8"][w]["ms"]["median"] / rec["b1"][w]["ms"]["median"], 3) for w in RUNS}
    for ix in arms.values():
        ix.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", help="m,n,k: one shape (k in bits)")
    ap.add_argument("--reps", type=int, default=0, help="passes per timed window (0: about 0.3 s of work, at most 20)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "b1_probe.json"))
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
