"""CPU tests of the lazy split filter on 16x16x32 MFMAs (OpLazySplit16, filter_lazy16_kernel): the compiled kernel
(one instantiation, no MFMA read hazards behind the inline-asm MFMAs, no scratch, <= 256 VGPRs, slot loops on
v_mfma_f32_16x16x32_bf16 with the counted ring wait and no full vmcnt drain — the refinement is laid out behind the
loop), the 32x32x16 lazy kernel still in the build, the operand gather (tools/lazy16_gather_check.cpp: a host program
over lazy16_gather of nns_internal.h), and the build's getter."""
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def isa():
    """(checker module, {kernel name: [(line number, text)]} of the lazy kernels, whole text) of ONE compilation."""
    spec = importlib.util.spec_from_file_location("check_mfma_hazards", os.path.join(ROOT, "tools", "check_mfma_hazards.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    with open(chk.compile_isa()) as f:
        text = f.read().splitlines()
    return chk, chk.split_kernels(text, r"filter_lazy(?:16)?_kernel", end=".Lfunc_end"), text


def test_one_lazy16_kernel_and_the_32x32_lazy_kernel_stays(isa):
    _, kernels, _ = isa
    assert len([k for k in kernels if "filter_lazy16_kernel" in k]) == 1, list(kernels)
    assert len([k for k in kernels if "filter_lazy_kernel" in k]) >= 1, list(kernels)


def test_lazy16_kernel_has_no_hazards_no_scratch_and_fits_256_vgprs(isa):
    chk, kernels, text = isa
    (name,) = [k for k in kernels if "filter_lazy16_kernel" in k]
    lines = kernels[name]
    body = [(i, l) for i, l in lines if "s_endpgm" not in l]
    assert chk.check_kernel(name, body) == []
    assert not any("scratch_" in l for _, l in lines)
    vg = [int(m.group(1)) for l in text for m in [re.match(r"\s*\.set " + re.escape(name) + r"\.num_vgpr, (\d+)", l)] if m]
    ag = [int(m.group(1)) for l in text for m in [re.match(r"\s*\.set " + re.escape(name) + r"\.num_agpr, (\d+)", l)] if m]
    assert len(vg) == 1 and len(ag) == 1, (vg, ag)
    print(f"filter_lazy16_kernel: {vg[0]} VGPRs, {ag[0]} AGPRs")
    assert vg[0] + ag[0] <= 256, (vg, ag)


def test_lazy16_slot_loops_run_16x16x32_with_a_counted_wait_and_never_drain_vmcnt(isa):
    _, kernels, _ = isa
    (name,) = [k for k in kernels if "filter_lazy16_kernel" in k]
    lines = [l for _, l in kernels[name]]
    assert not any("v_mfma_f32_32x32x16_bf16" in l for l in lines)
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
        if not closed or not any("v_mfma_f32_16x16x32_bf16" in b for b in body):
            continue
        loops += 1
        # one interval: 16 steps x 4 MFMAs; the refinement's MFMAs are not between the header and the back-edge
        assert sum("v_mfma_f32_16x16x32_bf16" in b for b in body) == 64, (m.group(1),)
        waits = [b.split(";")[0].strip() for b in body if re.match(r"\s*s_waitcnt\b", b)]
        counted = [w for w in waits if re.search(r"vmcnt\([1-9]\d*\)", w)]
        assert counted, (m.group(1), waits)                       # sync_slot's wait leaves the youngest pieces in flight
        assert [w for w in waits if re.search(r"vmcnt\(0\)", w)] == [], (m.group(1), waits)
    assert loops >= 1


def test_gather_offsets_and_lds_banks_host_program(tmp_path):
    exe = str(tmp_path / "lazy16_gather_check")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "nns-cuda_amd", "csrc"), os.path.join(ROOT, "tools", "lazy16_gather_check.cpp"),
                    "-o", exe], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    run = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout
    assert "lazy16_gather ok" in run.stdout


def test_default_build_runs_the_16x16_lazy_kernel(pkg):
    assert pkg.filter_lazy_tile() == 16
