"""The G2 bucket MSM without a device: the entry point's name, wrapper and refusals, and its plan (ezkl_amd/csrc/msm_plan.hpp: pick_plan_g2,
msm_plan_g2) as a plain program under AddressSanitizer and UndefinedBehaviorSanitizer -- tests/cpp/test_msm_g2_plan.cpp says what it asserts.
Nothing is loaded into the interpreter under a sanitizer."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ezkl_hip_msm_g2_points_dev"


def test_the_entry_point_is_declared_listed_once_exported_and_wrapped():
    from ezkl_amd import backend as B, lib as L
    header = open(os.path.join(ROOT, "include", "ezkl_hip.h")).read()
    assert re.search(r"int\s+%s\(const void\* points_dev, const void\* scalars_dev, size_t n, void\* out_affine, void\* stream\);" % NAME, header)
    assert 'ezkl_hip_last_kernel_ms("msm_g2")' in header
    assert L.SYMBOLS.count(NAME) == 1
    assert hasattr(L.load(), NAME)
    assert list(inspect.signature(B.msm_g2_points).parameters)[:2] == ["points", "scalars"]


def test_refusals_need_no_device_and_no_device_is_reported_not_computed():
    from ezkl_amd import lib as L
    f = getattr(L.load(), NAME)
    o, p = (C.c_uint64 * 16)(), C.c_void_p(0x1000)
    for args in ((None, p, 1, o), (p, None, 1, o), (p, p, 0, o), (p, p, 1, None), (C.c_void_p(0x1008), p, 1, o)):
        assert f(args[0], args[1], C.c_size_t(args[2]), args[3], None) == -3                     # EZKL_ERR_INVALID
    if L.load().ezkl_hip_device_count() > 0:                                                      # with a device the call would compute
        return
    assert f(p, p, C.c_size_t(1), o, None) == -1 and not any(o)                                   # EZKL_ERR_NO_DEVICE


def test_msm_g2_plan_under_the_sanitizers(tmp_path):
    from ezkl_amd import backend as B
    exe = str(tmp_path / "test_msm_g2_plan")
    cmd = ["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-std=c++17", "-Wall",
           "-Wextra", "-Werror", "-I", os.path.join(ROOT, "ezkl_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_msm_g2_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-6000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    print(r.stdout)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-2000:] + r.stderr[-6000:]
    for mark in ("Sanitizer", "runtime error"):
        assert mark not in r.stderr, r.stderr[-6000:]
    # the two sizes the Python side mirrors (the GPU tests pick their n by them)
    assert "crossover=%d sort_tile=%d\n" % (B.MSM_G2_CROSSOVER, B.MSM_G2_SORT_TILE) in r.stdout
