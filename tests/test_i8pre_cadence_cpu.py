"""CPU tests of the int8 pre-pass's barrier cadence (OpI8Pre: one workgroup barrier per kI8PreGroup intervals; DESIGN,
"Barrier cadence of the pre-pass"): the ring-safety predicate pre_cadence_ok of nns_internal.h against a brute force of the
protocol (tools/pre_cadence_check.cpp, a host program), and the kernels' listing — the counted wait in front of the slot
loop's barrier, and every other filter kernel's barriers as they were."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

# s_barrier instructions per kernel (label to .Lfunc_end) in a build of the commit before the cadence: the operators
# other than OpI8Pre keep kGroup = 1 and compile to the code they had
PARENT_BARRIERS = {
    "filter_lazy_kernel<OpLazySplitT<8,2>>": ("18filter_lazy_kernelINS_12OpLazySplitTILi8ELi2EEEEE", 6),
    "filter_lazy16_kernel<OpLazySplit16>": ("20filter_lazy16_kernelINS_13OpLazySplit16EEE", 2),
    "filter_i8_kernel<OpI8>": ("16filter_i8_kernelINS_4OpI8EEE", 2),
    "filter_f16_kernel<OpF16T<8>>": ("17filter_f16_kernelINS_6OpF16TILi8EEEEE", 2),
    "filter_f16_kernel<OpF16T<16>>": ("17filter_f16_kernelINS_6OpF16TILi16EEEEE", 2),
    "filter_kernel<OpBF16T<8,8,2>>": ("13filter_kernelINS_7OpBF16TILi8ELi8ELi2ELb0EEEEE", 2),
    "filter_kernel<OpBF16T<16,8,2>>": ("13filter_kernelINS_7OpBF16TILi16ELi8ELi2ELb0EEEEE", 2),
    "filter_kernel<OpBF16T32T<24,1,8>>": ("13filter_kernelINS_10OpBF16T32TILi24ELi1ELi8ELb0EEEEE", 7),
    "filter_kernel<OpBF16T<32,8,1>>": ("13filter_kernelINS_7OpBF16TILi32ELi8ELi1ELb0EEEEE", 2),
    "filter_kernel<OpBF16T32T<40,1,8>>": ("13filter_kernelINS_10OpBF16T32TILi40ELi1ELi8ELb0EEEEE", 11),
    "filter_kernel<OpBF16T32T<48,1,8>>": ("13filter_kernelINS_10OpBF16T32TILi48ELi1ELi8ELb0EEEEE", 7),
    "filter_kernel<OpBF16T32T<64,1,4>>": ("13filter_kernelINS_10OpBF16T32TILi64ELi1ELi4ELb0EEEEE", 5),
    "filter_split_kernel<OpSplitT<2,2>>": ("19filter_split_kernelINS_8OpSplitTILi2ELi2EEEEE", 3),
    "filter_split_kernel<OpSplitT<4,2>>": ("19filter_split_kernelINS_8OpSplitTILi4ELi2EEEEE", 5),
    "filter_split_kernel<OpSplitT<8,2>>": ("19filter_split_kernelINS_8OpSplitTILi8ELi2EEEEE", 6),
    "filter_split_kernel<OpSplitT<16,2>>": ("19filter_split_kernelINS_8OpSplitTILi16ELi2EEEEE", 6),
    "filter_split_kernel<OpSplitT<32,1>>": ("19filter_split_kernelINS_8OpSplitTILi32ELi1EEEEE", 7),
    "filter_kernel<OpF32T<2,2>>": ("13filter_kernelINS_6OpF32TILi2ELi2EEEEE", 3),
    "filter_kernel<OpF32T<4,2>>": ("13filter_kernelINS_6OpF32TILi4ELi2EEEEE", 5),
    "filter_kernel<OpF32T<8,2>>": ("13filter_kernelINS_6OpF32TILi8ELi2EEEEE", 5),
    "filter_kernel<OpF32T<16,2>>": ("13filter_kernelINS_6OpF32TILi16ELi2EEEEE", 6),
    "filter_kernel<OpF32T<32,1>>": ("13filter_kernelINS_6OpF32TILi32ELi1EEEEE", 7),
}


def _constants():
    """(ring depth, AHEAD, G) as nns_internal.h defines them for the default build"""
    text = open(os.path.join(ROOT, "nns-cuda_amd", "csrc", "nns_internal.h")).read()
    d = int(re.search(r"constexpr int kI8PreRingDepth = (\d+);", text).group(1))
    a = int(re.search(r"#define NNS_F_PRE_AHEAD (\d+)", text).group(1))
    g = int(re.search(r"#define NNS_F_PRE_GROUP (\d+)", text).group(1))
    return d, a, g


def _pieces_per_wave_and_slot():
    """F_PPS of the pre-pass ring as filter_mfma.hip lays it out: a slot's kSlotSteps 1 KiB fragments, one DMA piece each,
    dealt over the workgroup's kNW waves (OpI8Pre inherits OpBase's kNW and brings its seeds as one more piece of one wave,
    which the counted waits do not count)."""
    text = open(os.path.join(ROOT, "nns-cuda_amd", "csrc", "filter_mfma.hip")).read()
    base = text[text.index("struct OpBase {"):]
    base = base[:base.index("};")]
    pre = text[text.index("struct OpI8Pre :"):]
    pre = pre[:pre.index("};")]
    nw = int(re.search(r"static constexpr int kNW = (\d+);", base).group(1))
    assert "kNW" not in pre, "OpI8Pre has a workgroup size of its own: read it here"
    steps = int(re.search(r"static constexpr int kSlotSteps = (\d+);", pre).group(1))
    assert steps % nw == 0 and "constexpr int F_PPW = F_SLOT_COORD<OP> / 1024 / F_NW;" in text, (steps, nw)
    return steps // nw


def test_cadence_predicate_accepts_exactly_the_safe_combinations(tmp_path):
    """tools/pre_cadence_check.cpp: ring of 16, AHEAD 2 .. 15, G 1 .. 8, every pair of wave positions the barriers allow on
    streams from one slot to several ring turns — and the build's own (AHEAD, G)."""
    exe = str(tmp_path / "pre_cadence_check")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "nns-cuda_amd", "csrc"), os.path.join(ROOT, "tools", "pre_cadence_check.cpp"),
                    "-o", exe], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    run = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout
    d, a, g = _constants()
    assert "pre cadence ok" in run.stdout and f"build AHEAD {a} G {g}" in run.stdout, run.stdout
    # G = 2 and G = 4 with the lead of eight, and G = 4 with a lead up to twelve, are what the ring of sixteen admits
    ok = lambda aa, gg: gg < aa and aa + gg <= d   # noqa: E731
    assert ok(8, 2) and ok(8, 4) and ok(12, 4) and not ok(13, 4) and not ok(8, 8) and ok(a, g)


def test_listing_wait_in_front_of_the_loop_barrier_and_the_other_kernels_barriers():
    """Through tools/isa_report.py (the listing it names).  The s_waitcnt vmcnt in front of the pre-pass loop's barrier
    leaves (AHEAD - G - 1) F_PPS pieces in flight; every other filter kernel has as many s_barrier as before."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_mfma_hazards as chk
    rep = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_report.py")], check=True, stdout=subprocess.PIPE,
                         text=True).stdout.splitlines()
    text = open(rep[-1].strip()).read().splitlines()
    d, a, g = _constants()
    F_PPS = _pieces_per_wave_and_slot()
    kern = chk.split_kernels(text, which=r"filter_i8pre_kernel", end=".Lfunc_end")
    (lines,) = kern.values()
    body = [l.split(";")[0].strip() for _, l in lines]
    body = [l for l in body if l]
    bars = [j for j, l in enumerate(body) if l.startswith("s_barrier")]
    assert len(bars) == 2, bars                              # the prologue's and the slot loop's
    waits = []
    for b in bars:
        w = max(j for j in range(b) if body[j].startswith("s_waitcnt") and "vmcnt" in body[j])
        waits.append(int(re.search(r"vmcnt\((\d+)\)", body[w]).group(1)))
        assert not any(l.startswith(("global_load", "buffer_load", "global_store")) for l in body[w:b]), body[w:b]
    assert waits[1] == (a - g - 1) * F_PPS, (waits, a, g)
    assert waits[0] == ((a - 1) if g == 1 else (a - g - 1)) * F_PPS, (waits, a, g)   # the prologue: slots 0 .. G confirmed
    # the loop's barrier sits behind a scalar branch on the slot index alone (no barrier at all under G = 1's branch)
    if g > 1:
        assert body[bars[1] - 2].startswith("s_cbranch_scc") or body[bars[1] - 3].startswith("s_cbranch_scc"), body[bars[1] - 4:bars[1] + 1]
    other = chk.split_kernels(text, which=r"filter_\w*kernel", end=".Lfunc_end")
    seen = 0
    for name, (mangled, want) in PARENT_BARRIERS.items():
        hits = [v for k, v in other.items() if mangled in k]
        assert len(hits) == 1, (name, [k for k in other if mangled in k])
        got = sum(l.split(";")[0].strip().startswith("s_barrier") for _, l in hits[0])
        assert got == want, (name, got, want)
        seen += 1
    assert seen == len(other) - 1, sorted(other)             # every filter kernel but the pre-pass's is in the table
