#!/usr/bin/env python3
"""Per-kernel memory-instruction audit of a device source: compiles it for gfx950 to assembly (no GPU needed) and counts, per kernel, the
FLAT and GLOBAL memory instructions, the waits that drain both counters at once (s_waitcnt vmcnt(0) lgkmcnt(0)) and the counted vmcnt waits,
next to the VGPRs / scratch / occupancy the compiler reports.

    python tools/isa_audit.py ezkl_amd/csrc/msm.hip [more.hip ...] [--asm FILE.s]

A FLAT access counts on vmcnt AND lgkmcnt, so every LDS wait drains the global traffic as well; a kernel of the MSM chain must have none
(tests/test_msm_isa_cpu.py).  The usual cause is a device pointer that went through an integer."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S"]


def compile_asm(src, out):
    """-> the compiler's remarks (stderr) of the -S compile of `src` into `out`"""
    r = subprocess.run([HIPCC] + FLAGS + ["-Rpass-analysis=kernel-resource-usage", src, "-o", out], capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError(r.stderr[-4000:])
    return r.stderr


def demangle(names):
    try:
        out = subprocess.run(["c++filt", "-p"] + list(names), capture_output=True, text=True, check=True).stdout.split("\n")      # -p: no parameter lists
        return {n: re.sub(r"<.*", "", o.replace("(anonymous namespace)::", "")).split("::")[-1] or n for n, o in zip(names, out)}
    except Exception:
        return {n: n for n in names}


def kernels(asm_text):
    """-> {mangled kernel name: [instruction lines]} for every kernel (.amdhsa_kernel) of the assembly"""
    entry = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm_text, re.M))
    body, cur = {}, None
    for line in asm_text.split("\n"):
        m = re.match(r"^(\S+):", line)
        if m and m.group(1) in entry:
            cur = m.group(1)
            body[cur] = []
        elif cur is not None:
            if line.startswith(".Lfunc_end") or line.lstrip().startswith(".section"):
                cur = None
            else:
                body[cur].append(line.split(";")[0].strip())
    return body


def count(lines):
    c = {"flat": 0, "global": 0, "drain": 0, "vmcnt": 0}
    for ins in lines:
        if re.match(r"flat_(load|store|atomic)", ins):
            c["flat"] += 1
        elif re.match(r"global_(load|store|atomic)", ins):
            c["global"] += 1
        elif ins.startswith("s_waitcnt"):
            if "vmcnt(0)" in ins and "lgkmcnt(0)" in ins:
                c["drain"] += 1
            elif "vmcnt(" in ins:
                c["vmcnt"] += 1
    return c


def resources(remarks):
    """-> {mangled name: {vgprs, scratch, occupancy}} from -Rpass-analysis=kernel-resource-usage"""
    res, cur = {}, None
    for line in remarks.split("\n"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        if cur is None:
            continue
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m:
                cur[key] = int(m.group(1))
    return res


def audit(src, asm=None):
    with tempfile.TemporaryDirectory() as td:
        out = asm or os.path.join(td, "out.s")
        remarks = compile_asm(src, out)
        text = open(out).read()
    body, res = kernels(text), resources(remarks)
    names = demangle(sorted(body))
    rows = []
    for k in sorted(body, key=lambda k: names[k]):
        c = count(body[k])
        c.update(res.get(k, {}))
        rows.append((names[k], c))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("src", nargs="+")
    ap.add_argument("--asm", help="keep the assembly of the (single) source here")
    a = ap.parse_args()
    for src in a.src:
        print("%s\n%-44s %5s %6s %6s %6s %6s %7s %4s" % (src, "kernel", "flat", "global", "drains", "vmcnt", "VGPRs", "scratch", "occ"))
        for name, c in audit(src, a.asm if len(a.src) == 1 else None):
            print("%-44s %5d %6d %6d %6d %6s %7s %4s" % (name, c["flat"], c["global"], c["drain"], c["vmcnt"], c.get("vgprs", "?"), c.get("scratch", "?"), c.get("occupancy", "?")))
    return 0


if __name__ == "__main__":
    sys.exit(main())
