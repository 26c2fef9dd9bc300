#!/usr/bin/env python3
"""Kernel count, registers, spills and occupancy of every kernel in csrc/gtop_kernels.hip — the instantiations of
gtop_eval_wave_kernel (csrc/gtop_wave_kernel.h) its launchers select — (a CPU-side compile:
hipcc -Rpass-analysis=kernel-resource-usage); exits non-zero if any kernel spills — run by tests/test_capi.py, so a
compiler or flag change that pushes a body into scratch (the hand-issued loads of the latency variant depend on the
register allocator keeping their results where they land) is seen at build time.
usage: tools/kernel_resources.py [--asm-out FILE] [--source FILE.hip] [extra hipcc flags...]
       tools/kernel_resources.py --table                  (profiles/kernel_table.md: every body of both objects)
       tools/kernel_resources.py --compare OLD.s NEW.s    (two ISA listings kernel by kernel; non-zero if they differ)
--source names another file of csrc/ (gtop_validate.hip, gtop_edt.hip, gtop_setup.hip, ...); the default is
gtop_kernels.hip."""
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grad_traj_optimization_amd", "csrc")


def analyse(extra=(), asm_out="/tmp/gtop_kernels.s", source="gtop_kernels.hip"):
    """source: the file under csrc/ to compile (the default is the evaluation kernels' file)."""
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
           "-I" + CSRC, "-ffp-contract=on", "-mllvm", "-amdgpu-kernarg-preload-count=10", *extra, "-x", "hip",
           os.path.join(CSRC, source), "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-o", asm_out]
    t0 = time.time()
    out = subprocess.run(cmd, capture_output=True, text=True)
    secs = time.time() - t0
    if out.returncode != 0:
        raise RuntimeError(out.stderr[-2000:])
    rows = []
    for b in re.split(r"remark: Function Name: ", out.stderr)[1:]:
        name = b.split()[0]
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        dem = dem.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]

        def g(k):
            return int(re.search(k + r": (\d+)", b).group(1))
        rows.append(dict(kernel=dem, vgprs=g("VGPRs"), sgprs=g("TotalSGPRs"), scratch=g(r"ScratchSize \[bytes/lane\]"),
                         sgpr_spill=g("SGPRs Spill"), vgpr_spill=g("VGPRs Spill"),
                         waves_per_simd=g(r"Occupancy \[waves/SIMD\]")))
    return rows, secs


_VREG = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")


def _vregs(text):
    regs = set()
    for m in _VREG.finditer(text):
        if m.group(1) is not None:
            regs.add(int(m.group(1)))
        else:
            regs.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return regs


def check_asm_loads(asm_path):
    """The hand-issued distance-field loads (inline asm `global_load_dwordx4`, csrc/gtop_wave_kernel.h asm_load_pair) are
    invisible to the compiler's wait-count insertion: the kernel waits for them itself (gtop_wait_pairs).  That is sound
    only while NOTHING touches a load's destination registers between its issue and the s_waitcnt that covers it — a
    v_mov the register allocator inserts after a compiler or flag change would read registers that have not landed.
    This walks the ISA of every kernel: each inline-asm load's destination VGPRs are tracked from its issue until an
    `s_waitcnt vmcnt(k)` leaves at most k memory operations outstanding (memory operations complete in order, so the
    oldest are done first; compiler-issued loads and stores in between are counted as outstanding too, which only
    makes the check stricter), and any instruction that names one of them in between is a violation.
    Returns (number of hand-issued loads seen, list of violations)."""
    kernel, in_asm, pending, seen, bad = None, False, [], 0, []   # pending: (dest VGPRs or None, line no, text)
    with open(asm_path) as f:
        for no, raw in enumerate(f, 1):
            line = raw.strip() if raw.lstrip().startswith(";;#") else raw.split(";")[0].strip()
            if line.startswith(";;#ASMSTART"):
                in_asm = True
                continue
            if line.startswith(";;#ASMEND"):
                in_asm = False
                continue
            if not line:
                continue
            if re.match(r"^[A-Za-z_.$][\w.$]*:", line):
                if not line.startswith(".L"):        # a new function: nothing is in flight across it
                    kernel, pending = line.split(":")[0], []
                continue
            if line.startswith("."):
                continue
            op = line.split()[0]
            if op == "s_waitcnt":
                m = re.search(r"vmcnt\((\d+)\)", line)
                if m:
                    k = int(m.group(1))
                    pending = pending[len(pending) - k:] if 0 < k < len(pending) else ([] if k == 0 else pending)
                continue
            if op == "s_endpgm":
                pending = []
                continue
            touched = _vregs(line)
            for dest, pno, ptext in pending:
                if dest and dest & touched:
                    bad.append(f"{kernel}: line {no} `{line}` touches v{sorted(dest & touched)} of the load issued at "
                               f"line {pno} (`{ptext}`) before a wait covers it")
            if re.match(r"(global|flat|buffer|scratch)_(load|store|atomic)", op):
                if in_asm and op.startswith("global_load"):
                    seen += 1
                    pending.append((_vregs(line.split(",")[0]), no, line))
                else:
                    pending.append((None, no, line))
    return seen, bad


def table():
    """One markdown row per kernel of the two objects gtop_kernels.hip is compiled into."""
    ver = subprocess.run(["/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True).stdout
    print("Compiler: " + next(ln.strip() for ln in ver.splitlines() if "clang version" in ln))
    for title, extra in (("reference-mode object", ()), ("consistent-gradient object", ("-DGTOP_CONSISTENT_TU",))):
        rows, _ = analyse(extra, os.devnull)
        print(f"\n## {title}: {len(rows)} kernels\n\n| kernel | VGPRs | SGPRs | waves/SIMD | scratch |\n|---|---|---|---|---|")
        for r in rows:
            print(f"| `{r['kernel']}` | {r['vgprs']} | {r['sgprs']} | {r['waves_per_simd']} | {r['scratch']} |")
    return 0


# .LBB<n>_<k>, .LJTI<n>_<k>, .Lfunc_end<n>, and BB<n>_<k> in the loop comments
_LOCAL_LABEL = re.compile(r"(\.Lfunc_begin|\.Lfunc_end|\.L[A-Za-z]+(?=\d+_\d)|\bBB(?=\d+_\d))\d+")


def split_listing(text):
    """An ISA listing (hipcc -S --cuda-device-only) per function symbol: {name: {"text", "amdhsa", "metadata"}}, each a
    list of lines — the instruction text (labels, directives and the resource comments behind it included), the
    .amdhsa_kernel block and the kernel's entry in the metadata.  Lines that name the compilation unit's id
    (__hip_cuid_...) are dropped, and the function's ordinal in local labels is replaced: neither depends on the
    function's code, both on where and beside what it was compiled."""
    out, cur, part, in_meta, section = {}, None, "text", False, None
    for line in text.splitlines():
        if "__hip_cuid_" in line:
            continue
        line = re.sub(r"\s+;", " ;", _LOCAL_LABEL.sub(lambda m: m.group(1) + "N", line.rstrip()))   # (comment column: the label's width)
        if in_meta:
            if line.startswith("  - "):
                cur = []
            elif not line.startswith("    "):
                cur = None
            if cur is not None:
                cur.append(line)
                m = re.match(r"    \.name:\s+(\S+)", line)
                if m:
                    out.setdefault(m.group(1), {"text": [], "amdhsa": []})["metadata"] = cur
            continue
        if line.startswith("amdhsa.kernels:"):
            in_meta, cur = True, None
            continue
        m = re.search(r"; -- Begin function (\S+)", line)
        if m:
            if cur is not None and cur["text"] and cur["text"][-1] is section:
                cur["text"].pop()   # the .section line in front of a function is that function's
            cur, part = out.setdefault(m.group(1), {"text": [], "amdhsa": []}), "text"
            if section is not None:
                cur["text"].append(section)
        elif ".AMDGPU.gpr_maximums" in line:
            cur = None
        section = line if line.lstrip().startswith(".section") else None
        if cur is None:
            continue
        if line.lstrip().startswith(".amdhsa_kernel "):
            part = "amdhsa"
        cur[part].append(line)
        if line.lstrip().startswith(".end_amdhsa_kernel"):
            part = "text"
    return out


def compare_listings(old_text, new_text):
    """(kernels compared, names only in old, names only in new, {name: [parts that differ]})"""
    old, new = split_listing(old_text), split_listing(new_text)
    differ = {}
    for name in sorted(set(old) & set(new)):
        parts = [k for k in ("text", "amdhsa", "metadata") if old[name].get(k) != new[name].get(k)]
        if parts:
            differ[name] = parts
    return len(set(old) & set(new)), sorted(set(old) - set(new)), sorted(set(new) - set(old)), differ


def compare(old_path, new_path):
    n, only_old, only_new, differ = compare_listings(open(old_path).read(), open(new_path).read())
    print(f"{n} kernels compared, {len(differ)} differ, {len(only_old)} only in {old_path}, {len(only_new)} only in {new_path}")
    for tag, names in (("only old", only_old), ("only new", only_new)):
        for name in names:
            print(f"  {tag}: {name}")
    for name, parts in differ.items():
        print(f"  differs in {', '.join(parts)}: {name}")
    return 1 if differ or only_old or only_new else 0


def main():
    args = sys.argv[1:]
    if args[:1] == ["--table"]:
        return table()
    if args[:1] == ["--compare"] and len(args) == 3:
        return compare(args[1], args[2])
    asm_out = "/tmp/gtop_kernels.s"
    if args[:1] == ["--asm-out"]:
        asm_out, args = args[1], args[2:]
    source = "gtop_kernels.hip"
    if args[:1] == ["--source"]:
        source, args = args[1], args[2:]
    rows, secs = analyse(args, asm_out, source)
    bad = 0
    for r in rows:
        spill = r["scratch"] or r["vgpr_spill"]      # to memory; SGPR "spills" go to VGPR lanes (v_writelane), listed only
        bad += bool(spill)
        print(f"{r['vgprs']:4d} VGPR {r['sgprs']:4d} SGPR  {r['waves_per_simd']} waves/SIMD  "
              f"scratch {r['scratch']:3d}  spilled SGPR/VGPR {r['sgpr_spill']:3d}/{r['vgpr_spill']:<3d} {r['kernel'][:130]}"
              + ("   <== SCRATCH" if spill else ""))
    print(f"{len(rows)} kernels, compiled in {secs:.1f} s, {bad} use scratch memory")
    seen, viol = check_asm_loads(asm_out)
    print(f"{seen} hand-issued loads in the ISA, {len(viol)} touched before their wait")
    for v in viol[:20]:
        print("  " + v)
    return 1 if bad or viol else 0


if __name__ == "__main__":
    sys.exit(main())
