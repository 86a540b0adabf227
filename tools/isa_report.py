#!/usr/bin/env python3
"""Register / spill / v_mov report of the filter kernels' ISA (tuning aid); `isa_report.py b1`: the Hamming scans of
binary points instead (K1b, K6, K7 for b1_t); `isa_report.py u8`: K6's scan for int8 and uint8 points."""
import importlib.util, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("c", os.path.join(ROOT, "tools", "check_mfma_hazards.py"))
m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)


def b1_report():
    """`isa_report.py b1`: the binary-point (b1_t) instantiations of the lane-per-ref scans (K1b, K6, K7).  Per kernel the
    registers, and the census of its hottest loop (the innermost loop body with the most v_bcnt_u32_b32): xor, popcount,
    LDS reads and everything else, and from them the vector instructions per (query, word)."""
    import subprocess, tempfile
    csrc = os.path.join(ROOT, "nns-cuda_amd", "csrc")
    tmp = tempfile.mkdtemp(prefix="nns_isa_b1_")
    for src in ("exact_kernels", "topk_kernels", "range_kernels"):
        out = os.path.join(tmp, src + ".s")
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                        "-fno-slp-vectorize", "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only", "-o", out,
                        os.path.join(csrc, src + ".hip")], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        txt = open(out).read()
        lines = txt.splitlines()
        meta = {re.search(r"\.name:\s+(\S+)", b).group(1): b
                for b in re.findall(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", txt, flags=re.S)}
        for sym in [l.split(":")[0] for l in lines if l.startswith("_ZN3nns") and "@" in l and "4b1_t" in l]:
            start = next(i for i, l in enumerate(lines) if l.startswith(sym + ":"))
            end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
            body = [l.split(";")[0].strip() for l in lines[start:end]]
            # innermost loops: a backward branch to a label with no other label in between
            labels = {l[:-1]: i for i, l in enumerate(body) if re.fullmatch(r"\.LBB\d+_\d+:", l)}
            best = None
            for i, l in enumerate(body):
                mm = re.match(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)", l)
                if not mm or labels.get(mm.group(1), i) >= i:
                    continue
                loop = body[labels[mm.group(1)] + 1:i]
                if any(re.fullmatch(r"\.LBB\d+_\d+:", x) for x in loop):
                    continue
                n = sum(x.startswith("v_bcnt_u32_b32") for x in loop)
                if n and (best is None or n > best[0]):
                    best = (n, loop)
            g = lambda k: re.search(r"\.%s:\s+(\d+)" % k, meta[sym]).group(1)
            short = re.sub(r"^_ZN3nns\d+", "", sym)[:48]
            if best is None:
                print(short, "no popcount loop")
                continue
            n, loop = best
            cnt = lambda p: sum(x.startswith(p) for x in loop)
            valu = sum(x.startswith("v_") for x in loop)
            print(f"{short:48s} vgpr {g('vgpr_count')} spill {g('vgpr_spill_count')} | hot loop: {len(loop)} instr, "
                  f"v_bcnt {n}, v_xor {cnt('v_xor_b32')}, other VALU {valu - n - cnt('v_xor_b32')}, ds_read_b128 {cnt('ds_read_b128')}, "
                  f"ds_read_b32 {cnt('ds_read_b32') + cnt('ds_read2_b32')}, global_load {cnt('global_load')}, s_waitcnt {cnt('s_waitcnt')} "
                  f"-> {valu / n:.2f} VALU per (query, word)")
    print(tmp)


def bytes_report():
    """`isa_report.py u8`: the int8 (i8_t) and uint8 (u8_t) instantiations of K6's scan (topk_kernels.hip).  Per kernel the
    registers, and the census of its hottest loop (the innermost loop body with the most byte-to-float conversions): the
    row loads, the widening instructions (v_cvt_f32_ubyte0 .. 3 for uint8; v_bfe_i32 / shifts + v_cvt_f32_i32 for int8), and
    from them what the loop issues per 4 dimensions (= per 32-bit row load of the VEC 4 form)."""
    import subprocess, tempfile
    csrc = os.path.join(ROOT, "nns-cuda_amd", "csrc")
    tmp = tempfile.mkdtemp(prefix="nns_isa_u8_")
    out = os.path.join(tmp, "topk_kernels.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                    "-fno-slp-vectorize", "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only", "-o", out,
                    os.path.join(csrc, "topk_kernels.hip")], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    txt = open(out).read()
    lines = txt.splitlines()
    meta = {re.search(r"\.name:\s+(\S+)", b).group(1): b
            for b in re.findall(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", txt, flags=re.S)}
    conv = ("v_cvt_f32_ubyte", "v_cvt_f32_i32")
    for sym in [l.split(":")[0] for l in lines if l.startswith("_ZN3nns") and "@" in l and ("4i8_t" in l or "4u8_t" in l)]:
        start = next(i for i, l in enumerate(lines) if l.startswith(sym + ":"))
        end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
        body = [l.split(";")[0].strip() for l in lines[start:end]]
        labels = {l[:-1]: i for i, l in enumerate(body) if re.fullmatch(r"\.LBB\d+_\d+:", l)}
        best = None
        for i, l in enumerate(body):
            mm = re.match(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)", l)
            if not mm or labels.get(mm.group(1), i) >= i:
                continue
            loop = body[labels[mm.group(1)] + 1:i]
            if any(re.fullmatch(r"\.LBB\d+_\d+:", x) for x in loop):
                continue
            n = sum(x.startswith(conv) for x in loop)
            if n and (best is None or n > best[0]):
                best = (n, loop)
        g = lambda k: re.search(r"\.%s:\s+(\d+)" % k, meta[sym]).group(1)
        short = re.sub(r"^_ZN3nns\d+", "", sym)[:56]
        if best is None:
            print(short, "no conversion loop")
            continue
        n, loop = best
        cnt = lambda p: sum(x.startswith(p) for x in loop)
        valu = sum(x.startswith("v_") for x in loop)
        widen = cnt("v_cvt_f32_ubyte") + cnt("v_cvt_f32_i32") + cnt("v_bfe_i32") + cnt("v_ashrrev_i32") + cnt("v_lshlrev_b32")
        groups = n / 4.0                                  # 4-dimension groups the loop body widens
        print(f"{short:56s} vgpr {g('vgpr_count')} spill {g('vgpr_spill_count')} | hot loop: {len(loop)} instr, "
              f"global_load {cnt('global_load')}, v_cvt_f32_ubyte {cnt('v_cvt_f32_ubyte')}, v_cvt_f32_i32 {cnt('v_cvt_f32_i32')}, "
              f"v_bfe_i32 {cnt('v_bfe_i32')}, shifts {cnt('v_ashrrev_i32') + cnt('v_lshlrev_b32')}, VALU {valu}, "
              f"ds_read {cnt('ds_read')} -> per 4 dims: {widen / groups:.2f} widening, {valu / groups:.2f} VALU")
    print(tmp)


if len(sys.argv) > 1 and sys.argv[1] == "b1":
    b1_report()
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "u8":
    bytes_report()
    sys.exit(0)
path = m.compile_isa()
txt = open(path).read()
for b in re.findall(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", txt, flags=re.S):
    name = re.search(r"\.name:\s+(\S+)", b).group(1)
    if "filter_kernel" not in name and "filter_i8pre_kernel" not in name:   # (the int8 pre-pass: a kernel name of its own)
        continue
    g = lambda k: re.search(r"\.%s:\s+(\d+)" % k, b).group(1)
    print(name[20:62], "vgpr", g("vgpr_count"), "sgpr", g("sgpr_count"), "spill", g("vgpr_spill_count"), "scratch", g("private_segment_fixed_size"))
lines = txt.splitlines()
for sym in [l.split(":")[0] for l in lines if l.startswith(("_ZN3nns13filter_kernel", "_ZN3nns19filter_i8pre_kernel")) and "@" in l]:
    start = next(i for i, l in enumerate(lines) if l.startswith(sym + ":"))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    body = lines[start:end]
    run = best = 0
    for l in body:
        if "v_mov_b32" in l:
            run += 1; best = max(best, run)
        else:
            run = 0
    print(sym[20:62], len(body), "lines, v_mov", sum("v_mov_b32" in l for l in body), "longest run", best,
          "mfma", sum("v_mfma" in l for l in body), "barriers", sum("s_barrier" in l for l in body))
print(path)
