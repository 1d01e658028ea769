"""The plan of an MSM without window tables (ezkl_amd/csrc/msm_plan.hpp: pick_plan_once, msm_plan_once) and the identity that path computes
by -- signed digits, one sum per window, the host's combine -- as a plain program under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/cpp/test_msm_once_plan.cpp says what it asserts.  No device, no library loaded into the interpreter, no preload."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_msm_once_plan.cpp")
_FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "ezkl_amd", "csrc"), SRC]


def _run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, **kw)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    return r


def test_msm_once_plan_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "test_msm_once_plan")
    _run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] + _FLAGS + ["-o", exe])
    r = _run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert "all checks passed" in r.stdout
    for mark in ("Sanitizer", "runtime error"):
        assert mark not in r.stderr, r.stderr[-6000:]
