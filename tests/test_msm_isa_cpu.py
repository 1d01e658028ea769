"""The MSM chain's memory instructions, checked in the compiler's output (no GPU): ezkl_amd/csrc/msm.hip is compiled for gfx950 to assembly and
every kernel of the chain must address memory with GLOBAL instructions only and never wait on both counters at once.

Why it is a test: a FLAT access counts on vmcnt AND lgkmcnt, so with one in a kernel every wait for an LDS result also drains the outstanding
global loads and stores, and every wait for a load becomes the full drain `s_waitcnt vmcnt(0) lgkmcnt(0)` instead of a counted vmcnt(N).  One
cast of a device pointer through an integer (the batch shift `bshift` did that) or one pointer read from memory (the fused group's column list
was one) is enough to bring them back, the results stay right, and nothing else would notice."""
import os
import re
import shutil
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

CHAIN = ("msm_hist_kernel", "msm_hist_scan_kernel", "msm_part_scan_kernel", "msm_partition_kernel", "msm_binsort_kernel",
         "msm_bigsort_scatter_kernel", "msm_accumulate_kernel", "msm_fixup_boundary_tree_kernel", "msm_fixup_heavy1_kernel",
         "msm_fixup_heavy2_kernel", "msm_reduce1_kernel", "msm_reduce2_kernel", "msm_planes_kernel")

pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc is not installed")


@pytest.fixture(scope="module")
def kernel_bodies(tmp_path_factory):
    """{kernel name: its instructions} from one -S compile of msm.hip (about 20 s)"""
    out = str(tmp_path_factory.mktemp("isa") / "msm.s")
    src = os.path.join(ROOT, "ezkl_amd", "csrc", "msm.hip")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", src, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    text = open(out).read()
    entry = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    bodies, cur = {}, None
    for line in text.split("\n"):
        m = re.match(r"^(\S+):", line)
        if m and m.group(1) in entry:
            cur = m.group(1)
            bodies[cur] = []
        elif cur is not None:
            if line.startswith(".Lfunc_end"):
                cur = None
            else:
                ins = line.split(";")[0].strip()
                if ins:
                    bodies[cur].append(ins)
    named = {}
    for mangled, body in bodies.items():
        for k in CHAIN:
            if re.search(r"\d%s[A-Z]" % k, mangled):          # Itanium: <length><name>E...
                assert k not in named, (k, mangled)
                named[k] = body
    return named


def test_every_kernel_of_the_chain_was_found(kernel_bodies):
    assert sorted(kernel_bodies) == sorted(CHAIN)
    for k, body in kernel_bodies.items():
        assert any(i.startswith("s_endpgm") for i in body), k
        assert any(i.startswith("global_") for i in body), k        # each of them reads or writes HBM: the parser saw its body


@pytest.mark.parametrize("kernel", CHAIN)
def test_no_flat_memory_access(kernel_bodies, kernel):
    flat = [i for i in kernel_bodies[kernel] if re.match(r"flat_(load|store|atomic)", i)]
    assert not flat, "%s: %d flat accesses, e.g. %s" % (kernel, len(flat), flat[:3])


@pytest.mark.parametrize("kernel", CHAIN)
def test_no_wait_drains_both_counters(kernel_bodies, kernel):
    drains = [i for i in kernel_bodies[kernel] if i.startswith("s_waitcnt") and "vmcnt(0)" in i and "lgkmcnt(0)" in i]
    assert not drains, "%s: %d full drains (%s)" % (kernel, len(drains), drains[0])
