"""What the test_witness_plan_*_cpp.py drivers share: the blobs and the manifest a program of tests/cpp reads, and that program built as a plain
executable under AddressSanitizer and UndefinedBehaviorSanitizer and run.  No device, no library loaded into the interpreter, no preload."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "ezkl_amd", "csrc")]
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, **kw)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    return r


def build(tmp_path, name, flags=()):
    """tests/cpp/<name>.cpp -> the executable's path"""
    exe = str(tmp_path / name)
    run(["g++"] + list(flags) + FLAGS + [os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe])
    return exe


def parser_program(tmp_path, name, good, bad, ends_with=True):
    """the plans of `good`, and those of `bad` -- (words, record, plan), each refused by the Python validator with a message that ends with
    (ends_with=False: matches) `words` -- written with their manifest; tests/cpp/<name>.cpp built under the sanitizers and run on them"""
    from ezkl_amd import witness_plan as WP
    lines = []
    for i, plan in enumerate(good):
        (tmp_path / ("good_%d.bin" % i)).write_bytes(plan.validate().to_bytes())
        lines.append("good_%d.bin ok" % i)
    for i, (words, rec, plan) in enumerate(bad):
        with pytest.raises(WP.PlanError) as e:
            WP.validate(plan)
        assert str(e.value).endswith(words) if ends_with else re.search(words, str(e.value)), (str(e.value), words)
        (tmp_path / ("bad_%d.bin" % i)).write_bytes(plan.to_bytes())
        lines.append("bad_%d.bin bad %s" % (i, e.value))
    (tmp_path / "manifest.txt").write_text("\n".join(lines) + "\n")
    r = run([build(tmp_path, name, SANITIZE), str(tmp_path)], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert "all checks passed" in r.stdout
    for mark in ("Sanitizer", "runtime error"):
        assert mark not in r.stderr, r.stderr[-6000:]
