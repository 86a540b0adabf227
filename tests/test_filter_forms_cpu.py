"""The filter's plans, field for field, held against a recording of the library as it was before the operand-form table
(tests/golden/filter_plans_parent.json): all sixteen ints of nns_plan_filter (or its status) over five point types, the
operand and record flags, the k values around every tile depth and five (m, n) shapes from tiny to the flagship's; and over
the same k and shapes the flag-pass plans nns_plan_range_mfma{,_bf16,_u8} and nns_plan_topk_mfma{,_bf16,_u8} (kn 1 and
100).  Then the form table itself (nns_internal.h, kFilterForms), compiled from the header: each form's tau mode is the
one its public code stands for, nns_tau_consts at that mode gives the header's constants bit for bit, and every recorded
plan's kt and `bf16` field are its form's row.  No GPU is needed.

The recording is written by record() below from a library given by NNS_LIB_PATH (a build of the commit to record):
    NNS_LIB_PATH=/path/to/libnns_mi355x.so python tests/test_filter_forms_cpu.py
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "filter_plans_parent.json")

DTYPES = (0, 1, 2, 3, 5)            # fp32, bf16, fp16, int8, uint8
FLAG_PLAN_SUFFIX = {0: "", 1: "_bf16", 5: "_u8"}
PATH_MFMA, FILTER_BF16, RECORDS_PER_REF, FILTER_F32, SPLIT_EAGER = 2, 128, 512, 1024, 2048
FLAGS = (0, FILTER_BF16, FILTER_F32, SPLIT_EAGER, RECORDS_PER_REF, PATH_MFMA, SPLIT_EAGER | RECORDS_PER_REF)
KS = (8, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 384, 385, 512, 640, 641, 768, 769, 1024, 1025)
MN = ((1, 33), (64, 5003), (513, 65536), (1024, 1048576), (65536, 1048576))
FLAG_PLAN_FLAGS = (0, SPLIT_EAGER)
KNS = (1, 100)

# the operand forms by their public codes (nns_index_filter_form): what each row of kFilterForms must hold
FORM_TAU = (0, 1, 2, 3, 4, 1)       # TAU_F32, TAU_BF16, TAU_MIXED, TAU_SPLIT, TAU_F16, TAU_BF16
FORM_IMG_BYTES = (4, 2, 2, 4, 2, 1)
FORM_BF16 = (0, 1, 1, 0, 1, 1)      # nns_plan_filter's field 1
LADDER_F32 = (16, 32, 64, 128, 256)
LADDER_BF16 = (128, 256, 384, 512, 640, 768, 1024)
FORM_LADDER = (LADDER_F32, LADDER_BF16, LADDER_BF16, LADDER_F32, (128, 256), (256,))


def _filter_cases(dt):
    """(flags, k, m, n) of nns_plan_filter's grid for one dtype (NNS_PATH_MFMA: where it differs from AUTO, k > 256)"""
    return [(f, k, m, n) for f in FLAGS for k in KS if f != PATH_MFMA or k > 256 for m, n in MN]


def _flag_cases():
    return [(f, k, m, n) for f in FLAG_PLAN_FLAGS for k in KS for m, n in MN]


def _plan(fn, nout, *args):
    out = np.zeros(nout, np.int32)
    rc = fn(*args, out.ctypes.data, nout)
    return [int(rc)] if rc != 0 else [int(v) for v in out]


def _run_grid(pkg):
    """{"filter/<dtype>" | "range/<dtype>" | "topk<kn>/<dtype>": [one int list per case, [status] for a refusal]}"""
    L = pkg.lib
    grid = {}
    for dt in DTYPES:
        grid[f"filter/{dt}"] = [_plan(lambda *a: L.nns_plan_filter(k, m, n, dt, f, *a), 16) for f, k, m, n in _filter_cases(dt)]
    for dt, sfx in FLAG_PLAN_SUFFIX.items():
        rng, topk = getattr(L, "nns_plan_range_mfma" + sfx), getattr(L, "nns_plan_topk_mfma" + sfx)
        grid[f"range/{dt}"] = [_plan(lambda *a: rng(k, m, n, f, *a), 10) for f, k, m, n in _flag_cases()]
        for kn in KNS:
            grid[f"topk{kn}/{dt}"] = [_plan(lambda *a: topk(k, m, n, kn, f, *a), 17) for f, k, m, n in _flag_cases()]
    return grid


def record(path=GOLDEN):
    """Write the recording from the library NNS_LIB_PATH names (not collected; run on a build of the commit to record).
    A case is one int array; equal arrays are stored once ("rows") and a case names its row."""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    grid = _run_grid(pkg)
    rows = sorted({tuple(c) for cases in grid.values() for c in cases})
    number = {r: i for i, r in enumerate(rows)}
    with open(path, "w") as f:
        f.write("{\n")
        for key, val in (("library", os.path.basename(pkg.LIB_PATH)), ("dtypes", DTYPES), ("flags", FLAGS), ("k", KS),
                         ("mn", MN), ("flag_plan_flags", FLAG_PLAN_FLAGS), ("kn", KNS)):
            f.write(f" {json.dumps(key)}: {json.dumps(val)},\n")
        f.write(' "rows": [\n' + ",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in rows) + "\n ],\n")
        f.write(' "cases": {\n' + ",\n".join(f"  {json.dumps(k)}: {json.dumps([number[tuple(c)] for c in v], separators=(',', ':'))}"
                                             for k, v in grid.items()) + "\n }\n}\n")
    total = sum(len(v) for v in grid.values())
    print(f"{path}: {total} cases, {len(rows)} distinct arrays, {sum(len(r) == 1 for r in rows)} of them a bare status")


def _golden():
    with open(GOLDEN) as f:
        doc = json.load(f)
    assert (tuple(doc["dtypes"]), tuple(doc["flags"]), tuple(doc["k"]), tuple(map(tuple, doc["mn"])),
            tuple(doc["flag_plan_flags"]), tuple(doc["kn"])) == (DTYPES, FLAGS, KS, MN, FLAG_PLAN_FLAGS, KNS)
    rows = doc["rows"]
    return {key: [rows[i] for i in idx] for key, idx in doc["cases"].items()}


def test_every_plan_is_the_recorded_one(pkg):
    want = _golden()
    got = _run_grid(pkg)
    assert sorted(got) == sorted(want)
    bad = []
    for key in want:
        kind, dt = key.split("/")
        cases = _filter_cases(int(dt)) if kind == "filter" else _flag_cases()
        assert len(got[key]) == len(want[key]) == len(cases), key
        bad += [(key, c, g, w) for c, g, w in zip(cases, got[key], want[key]) if g != w]
    assert not bad, f"{len(bad)} cases differ; the first: {bad[:5]}"


def _form_of(dt, plan):
    """the operand form a recorded nns_plan_filter answer was granted: by dtype, then by its mixed / split / bf16 fields"""
    bf16, mixed, split = plan[1], plan[2], plan[14]
    return {2: 4, 3: 5, 5: 5}.get(dt, 2 if mixed else 3 if split else bf16)


def test_the_recorded_plans_follow_the_form_table():
    """every recorded filter plan: its tile depth is the first of its form's ladder that holds k, its `bf16` field the
    form's; every form is reached, and every depth of every ladder"""
    want = _golden()
    seen = set()
    for dt in DTYPES:
        for (flags, k, m, n), plan in zip(_filter_cases(dt), want[f"filter/{dt}"]):
            if len(plan) == 1:
                assert plan[0] != 0
                continue
            form = _form_of(dt, plan)
            assert (form in (0, 2, 3)) if dt == 0 else (form == {1: 1, 2: 4, 3: 5, 5: 5}[dt]), (dt, flags, k, plan)
            assert plan[0] == next(kt for kt in FORM_LADDER[form] if kt >= k), (dt, flags, k, plan)
            assert plan[1] == FORM_BF16[form] and plan[2] == (form == 2) and plan[14] == (form == 3), (dt, flags, k, plan)
            if plan[15]:   # the lazy schedule: split operands only
                assert form == 3
            seen.add((form, plan[0]))
    assert seen == {(form, kt) for form in range(6) for kt in FORM_LADDER[form]}


FORMS_SRC = r'''
#include <stdio.h>
#include "nns_internal.h"
int main()
{
    using namespace nns;
    static_assert(FORM_F32 == 0 && FORM_BF16 == 1 && FORM_MIXED == 2 && FORM_SPLIT == 3 && FORM_F16 == 4 && FORM_I8 == 5 &&
                      FORM_COUNT == 6, "the forms are nns_index_filter_form's public codes");
    for (int f = 0; f < FORM_COUNT; ++f) {
        const FilterForm &r = kFilterForms[f];
        printf("form %d %s %d %d %d", f, r.name, r.img_bytes, r.tau_mode, r.bf16);
        for (int kt : r.ladder)
            if (kt) printf(" %d", kt);
        printf("\n");
        for (int kt : r.ladder)
            if (kt) {
                const TauConsts t = tau_consts(kt, 10.7f, 3000.0f, r.tau_mode);
                printf("tau %d %d %a %a %a\n", f, kt, t.c0, t.c1, t.x2);
            }
    }
    const int dts[] = {DT_F32, DT_BF16, DT_F16, DT_I8, DT_B1, DT_U8};
    for (int dt : dts) printf("type %d %d\n", dt, kPointTypes[dt].filter_form);
    return 0;
}
'''


def test_the_form_table_and_its_tau_modes(pkg):
    """kFilterForms as the header compiles: names, image bytes, tau modes, the `bf16` plan field and the depth ladders are
    the documented rows; the point types' default forms; and nns_tau_consts at a form's tau mode returns, at every depth
    of the form's ladder, the constants the header gives the kernels, bit for bit"""
    from test_tau_model import _compile_host
    with tempfile.TemporaryDirectory() as d:
        exe = _compile_host(d, FORMS_SRC, "forms")
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    forms = [ln.split()[1:] for ln in out if ln.startswith("form ")]
    assert len(forms) == 6
    for f, row in enumerate(forms):
        assert int(row[0]) == f and row[1]
        assert (int(row[2]), int(row[3]), int(row[4])) == (FORM_IMG_BYTES[f], FORM_TAU[f], FORM_BF16[f]), row
        assert tuple(int(v) for v in row[5:]) == FORM_LADDER[f], row
    assert len({row[1] for row in forms}) == 6
    types = dict(tuple(int(v) for v in ln.split()[1:]) for ln in out if ln.startswith("type "))
    assert types == {0: 3, 1: 1, 2: 4, 3: 5, 4: -1, 5: 5}
    taus = [ln.split()[1:] for ln in out if ln.startswith("tau ")]
    assert len(taus) == sum(len(v) for v in FORM_LADDER)
    for f, kt, c0, c1, x2 in taus:
        got = pkg.tau_consts(int(kt), 10.7, 3000.0, FORM_TAU[int(f)])
        want = tuple(float(np.float32(float.fromhex(v))) for v in (c0, c1, x2))
        assert np.array_equal(np.float32(got).view(np.uint32), np.float32(want).view(np.uint32)), (f, kt, got, want)


if __name__ == "__main__":
    record()
