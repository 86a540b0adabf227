"""CPU tests around the lazy split filter's refinement path (lane thresholds shared inside the kernel, whatever the
schedule of the refinements): the PLAN does not move — every field nns_plan_filter reports for the shapes of
test_lazy_split_cpu.py::test_plans_report_the_lazy_schedule_where_enabled equals what the parent commit reported
(tests/golden/lazy_plans_parent.json, recorded from the parent's library; C3's values also spelled out here) — and the
lazy kernel's slot loops never wait with vmcnt(0): a full drain there also waits for the ring DMA pieces issued up to
AHEAD slots ahead.
(There is no NNS_F_LAZY_DEFER: deferred refinements were not built, DESIGN "Where the lazy kernel's time goes"; the
file keeps the name its issue gave it, and the vmcnt test guards the loop against any later scheduling change.)"""
import importlib.util
import json
import os
import re

from test_filter_cases_cpu import FILTER_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# nns_plan_filter(128, 65536, 1048576) of the parent commit, all 16 fields
C3_PLAN_PARENT = {
    "kt": 128, "bf16": 0, "mixed": 0, "lpq": 2, "m_pad": 65536, "n_pad": 1048576, "total_slots": 16384, "splits": 2,
    "slots_per_split": 8192, "qgroups": 128, "slot_pts": 64, "queries_per_wg": 512, "share_thr": 0, "tile_rec": 0,
    "split": 1, "lazy": 1,
}


def _shapes():
    shapes = [(9, 131072, 65537), (16, 250, 31), (17, 65536, 140001), (31, 250, 777), (64, 1000, 50000),
              (64, 65536, 1048576), (100, 65536, 1048576), (128, 65536, 1048576), (128, 200, 5000), (128, 70000, 300001),
              (200, 4096, 300001), (256, 250, 3001), (256, 65536, 1048576)]
    return shapes + [(c.k, c.m, c.n) for c in FILTER_CASES if c.dtype == "f32"]


def test_c3_plan_is_the_parents(pkg):
    p = pkg.plan_filter(128, 65536, 1048576, schedule=True)
    assert p == C3_PLAN_PARENT, p
    assert list(p) == list(C3_PLAN_PARENT)          # the fields' order too


def test_plans_are_the_parents(pkg, golden_dir):
    with open(os.path.join(golden_dir, "lazy_plans_parent.json")) as f:
        rec = json.load(f)
    want = {(e["k"], e["m"], e["n"], e["flags"]): e["plan"] for e in rec}
    checked = 0
    for k, m, n in _shapes():
        for name, flags in (("default", 0), ("per_ref", pkg.NNS_RECORDS_PER_REF), ("eager", pkg.NNS_FILTER_SPLIT_EAGER),
                            ("f32", pkg.NNS_FILTER_F32)):
            p = pkg.plan_filter(k, m, n, flags=flags, schedule=True)
            assert p == want[(k, m, n, name)], (k, m, n, name, p, want[(k, m, n, name)])
            checked += 1
    assert len(want) >= 4 * 13 and checked >= len(want)      # (a shape may appear twice in the list)


def test_lazy_slot_loops_never_drain_vmcnt():
    """In the ISA of every filter_lazy_kernel, between a slot loop's header and its back-edge: no s_waitcnt with
    vmcnt(0).  (The refinement is laid out behind the loop; a wait inside it counts ring pieces.)"""
    spec = importlib.util.spec_from_file_location("check_mfma_hazards", os.path.join(ROOT, "tools", "check_mfma_hazards.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    with open(chk.compile_isa()) as f:
        text = f.read().splitlines()
    kernels, cur = {}, None
    for l in text:
        m = re.match(r"^(_Z\w*filter_lazy_kernel\w*):", l)
        if m:
            cur = kernels.setdefault(m.group(1), [])
            continue
        if cur is not None:
            if l.startswith(".Lfunc_end"):
                cur = None
                continue
            cur.append(l)
    assert kernels
    for name, lines in kernels.items():
        loops = 0
        for idx, l in enumerate(lines):
            m = re.match(r"^(\.LBB\d+_\d+):.*Loop Header", l)
            if not m:
                continue
            body, closed = [], False
            for l2 in lines[idx + 1:]:
                body.append(l2)
                if re.search(r"s_cbranch_\w+\s+" + re.escape(m.group(1)) + r"\b", l2):
                    closed = True
                    break
            if not closed or not any("v_mfma_f32_32x32x16_bf16" in b for b in body):
                continue
            loops += 1
            waits = [b.split(";")[0].strip() for b in body if re.match(r"\s*s_waitcnt\b", b)]
            assert any("vmcnt(" in w for w in waits), (name, m.group(1))       # the counted wait of sync_slot is there
            drains = [w for w in waits if re.search(r"vmcnt\(0\)", w)]
            assert drains == [], (name, m.group(1), drains)
        assert loops >= 1, name
