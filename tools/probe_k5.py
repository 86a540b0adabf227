#!/usr/bin/env python3
"""K5 (finalize.hip, the unit-wise kernel) at C3: 65536 x 1048576 x 128 fp32, same device, same data.

usage: probe_k5.py ab libs A.so B.so   A/B of two BUILDS of the library (e.g. the parent commit's and this tree's): the
                                       builds alternate, 3 runs of 5 timed searches each, every run in a child process
                                       of its own (NNS_LIB_PATH).  finalize_ms (HIP events, NNS_PROFILE) and wall ms per
                                       search; the keys through their SHA-256, the sorted near-tie list through its
                                       SHA-256 and the ambiguous count must agree between the builds
       probe_k5.py stamps LIB.so       the sums of the per-wave stamps of a diagnostic build
                                       (tools/build_variant.sh <name> FINALIZE="-DNNS_DIAG [-DNNS_K5_SPARSE]"), one C3
                                       search in a child process with NNS_K5_STAMPS=1: s_memtime ticks of pass 1 (the
                                       minimum), of pass 2 as a whole and of the evaluations inside it, how many times
                                       the evaluation body ran per wave and with how many active lanes.  Read the
                                       SHARES: the stamps' fences make the diagnostic build slower than the product
       probe_k5.py c3 N                N C3 searches with the loaded library (rocprofv3 runs)
One JSON object per line on stdout."""
import hashlib
import json
import os
import subprocess
import sys
import time

M, N, K = 65536, 1048576, 128


def _child(lib, args, extra_env=None, stderr=None):
    env = dict(os.environ, NNS_LIB_PATH=os.path.abspath(lib), **(extra_env or {}))
    return subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, check=True, stdout=subprocess.PIPE,
                          stderr=stderr, text=True, timeout=300)


def ab_libs(libs):
    """(before the package is loaded: this process starts the children and never opens the device)"""
    res = {lib: {"finalize_ms": [], "wall_ms": []} for lib in libs}
    same = {lib: set() for lib in libs}
    for _ in range(3):
        for lib in libs:
            one = json.loads(_child(lib, ["librun", "5"]).stdout.strip().splitlines()[-1])
            res[lib]["finalize_ms"].append(one["finalize_ms"])
            res[lib]["wall_ms"].append(one["wall_ms"])
            res[lib]["ambiguous"] = one["ambiguous"]
            res[lib]["near_ties"] = one["near_ties"]
            same[lib].add((one["keys_sha256"], one["near_ties_sha256"], one["ambiguous"]))
    a, b = libs
    med = [sorted(res[lib]["finalize_ms"])[1] for lib in libs]
    print(json.dumps({"probe": "k5_ab_libs", "m": M, "n": N, "k": K, "a": a, "b": b, "arm_a": res[a], "arm_b": res[b],
                      "finalize_ms_median": med, "finalize_speedup_b_over_a": round(med[0] / med[1], 3),
                      "ranges_disjoint": {f: max(res[b][f]) < min(res[a][f]) for f in ("finalize_ms", "wall_ms")},
                      "keys_near_ties_ambiguous_equal": len(same[a] | same[b]) == 1}), flush=True)


def stamps(lib):
    out = _child(lib, ["c3", "2"], {"NNS_K5_STAMPS": "1"}, stderr=subprocess.PIPE)
    lines = [ln for ln in out.stderr.splitlines() if ln.startswith('{"k5_stamps"')]
    if not lines:
        raise SystemExit(f"{lib} printed no stamps: not a FINALIZE=-DNNS_DIAG build")
    s = json.loads(lines[-1])
    waves = s["units"]
    tot = s["pass1_ticks"] + s["pass2_ticks"]
    s.update({"probe": "k5_stamps", "lib": lib, "m": M, "n": N, "k": K,
              "share_pass1": round(s["pass1_ticks"] / tot, 3),
              "share_pass2_walk": round((s["pass2_ticks"] - s["eval_ticks"]) / tot, 3),
              "share_pass2_eval": round(s["eval_ticks"] / tot, 3),
              "eval_rounds_per_wave": round(s["eval_rounds"] / waves, 2),
              "active_lanes_per_round": round(s["eval_active_lanes"] / max(s["eval_rounds"], 1), 2),
              "candidates_per_wave": round(s["eval_active_lanes"] / waves, 2),
              "wave_us_mean": round(s["wave_realtime_ticks_100mhz"] / waves * 0.01, 2)})
    print(json.dumps(s), flush=True)


if __name__ == "__main__" and sys.argv[1:3] == ["ab", "libs"]:
    if len(sys.argv) != 5:
        raise SystemExit("usage: probe_k5.py ab libs A.so B.so")
    ab_libs(sys.argv[3:5])
    sys.exit(0)
if __name__ == "__main__" and sys.argv[1:2] == ["stamps"]:
    if len(sys.argv) != 3:
        raise SystemExit("usage: probe_k5.py stamps LIB.so")
    stamps(sys.argv[2])
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402

pkg = graft.load_package()


def _c3_index():
    q = torch.empty((M, K), dtype=torch.float32, device="cuda")
    r = torch.empty((N, K), dtype=torch.float32, device="cuda")
    pkg.fill_uniform(q, 1000, 0)
    pkg.fill_uniform(r, 1000, M * K)
    p = pkg.plan_filter(K, M, N)
    assert p["splits"] < 4 and p["tile_rec"] == 0, p       # the unit-wise kernel
    ix = pkg.Index(r, path="mfma", profile=True)
    keys = torch.empty(M, dtype=torch.int64, device="cuda")
    ix.search_keys(q, keys)                               # warm-up
    torch.cuda.synchronize()
    return ix, q, keys


def _timed(ix, q, keys, steps):
    ix.stats()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ix.search_keys(q, keys)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def librun(steps):
    """one run of `ab libs`: the library NNS_LIB_PATH names, default flags"""
    ix, q, keys = _c3_index()
    wall = _timed(ix, q, keys, steps)
    st = ix.stats()
    ties = ix.near_ties()
    print(json.dumps({"probe": "k5_librun", "wall_ms": round(wall, 3), "finalize_ms": round(st["finalize_ms"], 4),
                      "filter_ms": round(st["filter_ms"], 3), "ambiguous": st["ambiguous"], "near_ties": int(ties.size),
                      "keys_sha256": hashlib.sha256(keys.cpu().numpy().tobytes()).hexdigest(),
                      "near_ties_sha256": hashlib.sha256(np.ascontiguousarray(ties).tobytes()).hexdigest()}), flush=True)
    ix.close()


def c3(steps):
    ix, q, keys = _c3_index()
    wall = _timed(ix, q, keys, steps)
    print(json.dumps({"probe": "k5_c3", "steps": steps, "wall_ms": round(wall, 3),
                      "finalize_ms": round(ix.stats()["finalize_ms"], 4)}), flush=True)
    ix.close()


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    if what == "librun":
        librun(int(sys.argv[2]))
    elif what == "c3":
        c3(int(sys.argv[2]))
    else:
        raise SystemExit(__doc__)
