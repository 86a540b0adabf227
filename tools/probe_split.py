#!/usr/bin/env python3
"""Split-bf16 vs fp32 filter operands (fp32 points), same device, same data.

usage: probe_split.py ab [k ...]      per-depth A/B at 65536 x 1048576 (default k = 16 32 64 128 256): the two forms
                                      alternate, 3 runs of 5 timed searches each; filter_ms (HIP events, NNS_PROFILE) and
                                      wall ms per search, keys of the two forms compared bit for bit
       probe_split.py ab lazy [k ...] the same A/B of the split operands' two schedules: lazy (the default where the library
                                      enables it) against eager (NNS_FILTER_SPLIT_EAGER); default k = 128
       probe_split.py ab libs A.so B.so [k]
                                      the same protocol between two BUILDS of the library (e.g. the parent commit's and
                                      this tree's, or tools/build_variant.sh arms) at 65536 x 1048576 x k (default 128):
                                      the builds alternate, 3 runs of 5 timed searches each, every run in a child process
                                      of its own (NNS_LIB_PATH), keys compared through their SHA-256.  The lazy kernel on
                                      32x32x16 against 16x16x32 MFMAs: A = a `tools/build_variant.sh lazy32 -DNNS_F_LAZY_T16=0`
                                      build (or the commit before OpLazySplit16), B = the default build
       probe_split.py c3 split|f32 N  N C3 searches (65536 x 1048576 x 128) of one form (rocprofv3 / PMC runs)
       probe_split.py cluster         tight Gaussian clusters at 65536 x 1048576 x 128: exact-scan (ambiguous) and
                                      multi-candidate queries of each operand form
       probe_split.py denorm          does v_mfma_f32_32x32x16_bf16 flush bf16 denormal operands? (MFMA self-test)
One JSON object per line on stdout."""
import json
import os
import sys
import time

import numpy as np
import torch


def ab_libs(libs, k):
    """(before the package is loaded: this process starts the children and never opens the device)"""
    import subprocess
    res = {lib: {"wall_ms": [], "filter_ms": []} for lib in libs}
    sha = {}
    for _ in range(3):
        for lib in libs:
            env = dict(os.environ, NNS_LIB_PATH=os.path.abspath(lib))
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "librun", str(k), "5"], env=env, check=True,
                                 stdout=subprocess.PIPE, text=True, timeout=300).stdout
            one = json.loads(out.strip().splitlines()[-1])
            res[lib]["wall_ms"].append(one["wall_ms"])
            res[lib]["filter_ms"].append(one["filter_ms"])
            res[lib]["ambiguous"] = one["ambiguous"]
            res[lib]["form"] = one["form"]
            sha.setdefault(lib, set()).add(one["keys_sha256"])
    a, b = libs
    med = {lib: sorted(res[lib]["filter_ms"])[1] for lib in libs}
    print(json.dumps({"probe": "ab_libs", "m": 65536, "n": 1048576, "k": k, "a": a, "b": b, "arm_a": res[a], "arm_b": res[b],
                      "filter_ms_median": [med[a], med[b]], "filter_speedup_b_over_a": round(med[a] / med[b], 4),
                      "keys_equal": len(sha[a] | sha[b]) == 1}), flush=True)


if __name__ == "__main__" and sys.argv[1:3] == ["ab", "libs"]:
    if len(sys.argv) not in (5, 6):
        raise SystemExit("usage: probe_split.py ab libs A.so B.so [k]")
    ab_libs(sys.argv[3:5], int(sys.argv[5]) if len(sys.argv) > 5 else 128)
    sys.exit(0)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402

pkg = graft.load_package()
M, N = 65536, 1048576


def uniform(m, n, k, seed=1000):
    q = torch.empty((m, k), dtype=torch.float32, device="cuda")
    r = torch.empty((n, k), dtype=torch.float32, device="cuda")
    pkg.fill_uniform(q, seed, 0)
    pkg.fill_uniform(r, seed, m * k)
    return q, r


def timed(ix, q, keys, steps):
    ix.stats()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ix.search_keys(q, keys)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / steps * 1e3
    st = ix.stats()
    return wall, st["filter_ms"], st


def ab(ks, lazy=False):
    # (lazy: "split" = the default schedule, "f32" = the partner arm, here the eager split schedule)
    for k in ks:
        q, r = uniform(M, N, k)
        partner = {"filter_split_eager": True} if lazy else {"filter_f32": True}
        ixs = {f: pkg.Index(r, path="mfma", profile=True, **(partner if f == "f32" else {})) for f in ("split", "f32")}
        keys = {f: torch.empty(M, dtype=torch.int64, device="cuda") for f in ixs}
        for f, ix in ixs.items():
            ix.search_keys(q, keys[f])
        res = {f: {"wall_ms": [], "filter_ms": []} for f in ixs}
        for _ in range(3):
            for f, ix in ixs.items():
                w, fm, st = timed(ix, q, keys[f], 5)
                res[f]["wall_ms"].append(round(w, 3))
                res[f]["filter_ms"].append(round(fm, 3))
                res[f]["ambiguous"] = st["ambiguous"]
                res[f]["form"] = st["filter_form"]
        same = bool(torch.equal(keys["split"], keys["f32"]))
        fs, ff = np.median(res["split"]["filter_ms"]), np.median(res["f32"]["filter_ms"])
        if lazy:
            res = {"lazy": res["split"], "eager": res["f32"]}
            res["lazy"]["lazy_planned"] = pkg.plan_filter(k, M, N, schedule=True)["lazy"]
        print(json.dumps({"probe": "ab_lazy" if lazy else "ab", "m": M, "n": N, "k": k, "kt": ixs["split"].stats()["k_tile"], **res,
                          "filter_speedup_median": round(float(ff / fs), 3), "keys_equal": same}), flush=True)
        for ix in ixs.values():
            ix.close()
        del q, r
        torch.cuda.empty_cache()


def librun(k, steps):
    """one run of `ab libs`: the library NNS_LIB_PATH names, default flags"""
    import hashlib
    q, r = uniform(M, N, k)
    ix = pkg.Index(r, path="mfma", profile=True)
    keys = torch.empty(M, dtype=torch.int64, device="cuda")
    ix.search_keys(q, keys)
    w, fm, st = timed(ix, q, keys, steps)
    print(json.dumps({"probe": "librun", "k": k, "wall_ms": round(w, 3), "filter_ms": round(fm, 3), "ambiguous": st["ambiguous"],
                      "form": st["filter_form"], "keys_sha256": hashlib.sha256(keys.cpu().numpy().tobytes()).hexdigest()}),
          flush=True)
    ix.close()


def c3(form, steps):
    q, r = uniform(M, N, 128)
    ix = pkg.Index(r, path="mfma", filter_f32=(form == "f32"))
    keys = torch.empty(M, dtype=torch.int64, device="cuda")
    ix.search_keys(q, keys)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ix.search_keys(q, keys)
    torch.cuda.synchronize()
    print(json.dumps({"probe": "c3", "form": form, "steps": steps,
                      "wall_ms": round((time.perf_counter() - t0) / steps * 1e3, 3)}), flush=True)
    ix.close()


def clustered(m, n, k, clusters, sigma, seed=5):
    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = torch.rand((clusters, k), generator=g, device="cuda")
    rc = torch.randint(0, clusters, (n,), generator=g, device="cuda")
    qc = torch.randint(0, clusters, (m,), generator=g, device="cuda")
    r = (centres[rc] + sigma * torch.randn((n, k), generator=g, device="cuda")).contiguous()
    q = (centres[qc] + sigma * torch.randn((m, k), generator=g, device="cuda")).contiguous()
    return q, r


def cluster():
    for sigma in (0.03, 0.01, 0.003):
        q, r = clustered(M, N, 128, 1024, sigma)
        out = {}
        keys0 = None
        for f, kw in (("split", {}), ("split_eager", {"filter_split_eager": True}), ("f32", {"filter_f32": True}),
                      ("bf16", {"filter_bf16": True})):
            ix = pkg.Index(r, path="mfma", profile=True, **kw)
            keys = ix.search_keys(q)
            torch.cuda.synchronize()
            fms = [timed(ix, q, keys, 3)[1] for _ in range(3)]
            st = ix.stats()
            out[f] = {"ambiguous": st["ambiguous"], "multi_candidate": st["multi_candidate"],
                      "filter_ms": [round(x, 3) for x in fms]}
            if keys0 is None:
                keys0 = keys.clone()
            else:
                out[f]["keys_equal_split"] = bool(torch.equal(keys, keys0))
            ix.close()
        print(json.dumps({"probe": "cluster", "m": M, "n": N, "k": 128, "clusters": 1024, "sigma": sigma, **out}),
              flush=True)
        del q, r
        torch.cuda.empty_cache()


def denorm():
    kt = 16
    a = np.zeros((32, kt), np.float32)
    b = np.zeros((32, kt), np.float32)
    a[:, 0] = np.float32(2.0 ** -130)          # a bf16 denormal (exact in bf16: 2^-133 spacing)
    b[:, 0] = np.float32(2.0 ** 100)           # product 2^-30: far above FLT_MIN
    a[:, 1] = np.float32(2.0 ** -100)          # normal x normal with a product below FLT_MIN (2^-140)
    b[:, 1] = np.float32(2.0 ** -40)
    out = pkg.selftest_mfma(a, b, np.zeros(32, np.float32), bf16=1)
    a2 = np.zeros((32, kt), np.float32)
    a2[:, 1] = a[:, 1]
    b2 = np.zeros((32, kt), np.float32)
    b2[:, 1] = b[:, 1]
    out2 = pkg.selftest_mfma(a2, b2, np.zeros(32, np.float32), bf16=1)
    print(json.dumps({"probe": "denorm", "denormal_operand_product": float(out[0, 0]), "expected_if_kept": 2.0 ** -30,
                      "flushes_denormal_operands": bool(abs(float(out[0, 0])) < 2.0 ** -100),
                      "subnormal_product_alone": float(out2[0, 0]), "expected_subnormal": 2.0 ** -140,
                      "flushes_subnormal_products": bool(out2[0, 0] == 0)}), flush=True)


if __name__ == "__main__":
    what = sys.argv[1]
    if what == "ab":
        if sys.argv[2:3] == ["lazy"]:
            ab([int(x) for x in sys.argv[3:]] or [128], lazy=True)
        else:
            ab([int(x) for x in sys.argv[2:]] or [16, 32, 64, 128, 256])
    elif what == "librun":
        librun(int(sys.argv[2]), int(sys.argv[3]))
    elif what == "c3":
        c3(sys.argv[2], int(sys.argv[3]))
    elif what == "cluster":
        cluster()
    elif what == "denorm":
        denorm()
    else:
        raise SystemExit(__doc__)
