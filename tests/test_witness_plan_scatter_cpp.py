"""The C++ parser's SCATTER, COMPLEMENT and ONEHOT rules (ezkl_amd/csrc/witness_plan.hpp) as a plain program under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/cpp/test_witness_plan_scatter.cpp reads the blobs written here -- synthetic plans of the new kinds it must
take, the plan recorded from a ScatterGatherCircuit, and every plan of witness_synth_scatter.bad_plans() with the message the Python
validator gave for it -- and says what it asserts.  No device, no library loaded into the interpreter, no preload."""
import os
import subprocess

import pytest

import witness_synth_scatter as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_witness_plan_scatter.cpp")
_FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "ezkl_amd", "csrc"), SRC]
GOOD = ["scatter-n1", "scatter-n2", "scatter-n65", "scatter-n257", "complement-n1", "complement-n2", "complement-n64", "complement-n257", "onehot-edges", "onehot-outside"]


def _run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, **kw)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    return r


def test_the_indexed_rules_of_the_parser_under_the_sanitizers(tmp_path):
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    recorded = [WP.record_plan(EL.ScatterGatherCircuit(10, 2, 6000))]
    plans = ([T.small_plan().plan, T.failing_case(100, True).plan, T.failing_case(T.TILE + 1, True).plan, T.CASES["complement-n%d" % (T.TILE + 1)](1).plan] + recorded +
             [T.CASES[name](1).plan for name in GOOD])
    lines = []
    for i, plan in enumerate(plans):
        (tmp_path / ("good_%d.bin" % i)).write_bytes(plan.validate().to_bytes())
        lines.append("good_%d.bin ok" % i)
    for i, (words, rec, plan) in enumerate(T.bad_plans()):
        with pytest.raises(WP.PlanError) as e:
            WP.validate(plan)
        assert str(e.value).endswith(words)
        (tmp_path / ("bad_%d.bin" % i)).write_bytes(plan.to_bytes())
        lines.append("bad_%d.bin bad %s" % (i, e.value))
    (tmp_path / "manifest.txt").write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "test_witness_plan_scatter")
    _run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] + _FLAGS + ["-o", exe])
    r = _run([exe, str(tmp_path)], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert "all checks passed" in r.stdout
    for mark in ("Sanitizer", "runtime error"):
        assert mark not in r.stderr, r.stderr[-6000:]
