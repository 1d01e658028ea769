"""The MSM's host-side launch plan (ezkl_amd/csrc/msm_plan.hpp: the window plan, the launch geometry of the chain and the scratch layout, one
pure function of the size, the device shape and the tuning) built as a plain program under AddressSanitizer and UndefinedBehaviorSanitizer and
swept over sizes, device shapes, group sizes and tuning values: tests/cpp/test_msm_plan.cpp says what it asserts.  No device, no library
loaded into the interpreter, no preload."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_msm_plan.cpp")
_FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "ezkl_amd", "csrc"), SRC]


def _run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, **kw)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    return r


def test_msm_plan_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "test_msm_plan")
    _run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] + _FLAGS + ["-o", exe])
    r = _run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert "all checks passed" in r.stdout
    for mark in ("Sanitizer", "runtime error"):
        assert mark not in r.stderr, r.stderr[-6000:]
