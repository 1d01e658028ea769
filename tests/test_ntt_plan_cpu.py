"""The NTT planner (ezkl_amd/csrc/ntt.hip: plan_radices, plan_log_tile, pass_threads) read through ezkl_hip_ntt_plan_info, which needs no
device: invariants of every plan for every accepted EZKL_NTT_MAXR, agreement with the Python model of the pass (tools/ntt29_model.py), and
the literal plans tests/test_gpu_ntt_plans.py relies on -- a planner change that moves a GPU case off the kernel instance it was written
for fails here, on the CPU."""
import ctypes as C
import os
import sys

import pytest
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import ntt29_model as M
from ezkl_amd import backend as B, lib as L

LDS_LIMIT = 160 * 1024                      # what ntt_kernel_attrs requests for every instance of ntt_pass_kernel
LOG_NS = range(0, 29)
MAX_RADICES = range(6, 12)


def test_backend_and_raw_words_agree():
    out = (C.c_uint32 * 16)()
    assert L.load().ezkl_hip_ntt_plan_info(C.c_uint32(21), C.c_uint32(11), out) == 0
    assert list(out) == [2, 11, 10, 0, 0, 11, 12, 0, 0, 512, 1024, 0, 0, 11, 0, 0]
    assert B.ntt_plan_info(21, 11) == dict(npass=2, log_radix=[11, 10], log_tile=[11, 12], threads=[512, 1024], max_radix=11)


@pytest.mark.parametrize("log_n,max_radix", [(29, 8), (12, 5), (12, 12), (12, 1 << 31)])
def test_refuses_what_no_launch_would_take(log_n, max_radix):
    out = (C.c_uint32 * 16)()
    assert L.load().ezkl_hip_ntt_plan_info(C.c_uint32(log_n), C.c_uint32(max_radix), out) == -3        # EZKL_ERR_INVALID
    assert L.load().ezkl_hip_ntt_plan_info(C.c_uint32(12), C.c_uint32(8), None) == -3


@pytest.mark.parametrize("max_radix", MAX_RADICES)
def test_every_plan_is_launchable(max_radix):
    for log_n in LOG_NS:
        p = B.ntt_plan_info(log_n, max_radix)
        what = (log_n, max_radix, p)
        assert p["max_radix"] == max_radix
        assert sum(p["log_radix"]) == log_n, what
        assert (p["npass"] == 1) == (log_n <= 11) and 1 <= p["npass"] <= 4, what
        assert len(p["log_radix"]) == len(p["log_tile"]) == len(p["threads"]) == p["npass"]
        for log_r, log_tile, threads in zip(p["log_radix"], p["log_tile"], p["threads"]):
            assert log_r >= 1 or log_n == 0, what
            assert log_r <= log_tile <= log_n, what                       # whole tiles: the grid is 2^(log_n - log_tile) of them
            assert 36 * (1 << log_tile) + 36 * (1 << min(log_r, 6)) <= LDS_LIMIT, what
            assert threads in (256, 512, 1024), what
            if p["npass"] > 1:
                # every pass of a multi-pass plan is meant to take the unrolled four-elements-per-lane load and store
                assert 4 * threads == 1 << log_tile, what
            else:
                assert threads == 256, what                               # one pass: 256 lanes loop over the tile (unrolled at 2^10 only)


@pytest.mark.parametrize("max_radix", MAX_RADICES)
def test_planner_equals_the_python_model(max_radix):
    for log_n in LOG_NS:
        p = B.ntt_plan_info(log_n, max_radix)
        assert p["log_radix"] == M.plan_radices(log_n, max_radix), (log_n, max_radix)
        assert p["log_tile"] == [M.plan_log_tile(log_n, p["npass"], r) for r in p["log_radix"]], (log_n, max_radix)


def test_environment_value_in_force(monkeypatch):
    """max_radix = 0 reports what the process read from EZKL_NTT_MAXR (8 without it, or with a value outside 6..11), and reads it once"""
    env = os.environ.get("EZKL_NTT_MAXR", "")
    want = int(env) if env.isdigit() and 6 <= int(env) <= 11 else 8
    assert B.ntt_plan_info(13)["max_radix"] == want
    monkeypatch.setenv("EZKL_NTT_MAXR", "6" if want != 6 else "9")        # too late: the library keeps what it read first
    assert B.ntt_plan_info(13) == B.ntt_plan_info(13, want)


# (log_n, max radix) -> (radices, workgroup sizes): the plans the GPU tests are written for
PLANS = {
    # default plans: forward / scaled inverse / coset pairs / strided batches of tests/test_gpu_ntt_plans.py
    (3, 8): ([3], [256]), (5, 8): ([5], [256]), (9, 8): ([9], [256]), (10, 8): ([10], [256]), (11, 8): ([11], [256]),
    (12, 8): ([6, 6], [256, 256]), (13, 8): ([7, 6], [256, 256]), (14, 8): ([7, 7], [256, 256]), (15, 8): ([8, 7], [256, 256]),
    (16, 8): ([8, 8], [256, 256]), (17, 8): ([6, 6, 5], [256] * 3), (18, 8): ([6, 6, 6], [256] * 3), (19, 8): ([7, 6, 6], [256] * 3),
    (20, 8): ([7, 7, 6], [256] * 3), (21, 8): ([7, 7, 7], [256] * 3), (23, 8): ([8, 8, 7], [256] * 3),
    (25, 8): ([7, 6, 6, 6], [256] * 4),                                   # where four passes start by default
    # EZKL_NTT_MAXR variants
    (11, 6): ([11], [256]), (13, 6): ([5, 4, 4], [256] * 3), (15, 6): ([5, 5, 5], [256] * 3), (17, 6): ([6, 6, 5], [256] * 3),
    (18, 6): ([6, 6, 6], [256] * 3), (19, 6): ([5, 5, 5, 4], [256] * 4), (20, 6): ([5, 5, 5, 5], [256] * 4),
    (13, 7): ([7, 6], [256, 256]), (15, 7): ([5, 5, 5], [256] * 3), (20, 7): ([7, 7, 6], [256] * 3), (22, 7): ([6, 6, 5, 5], [256] * 4),
    (15, 9): ([8, 7], [256, 256]), (16, 9): ([8, 8], [256, 256]), (17, 9): ([9, 8], [512, 256]), (18, 9): ([9, 9], [512, 512]),
    (17, 10): ([9, 8], [512, 256]), (18, 10): ([9, 9], [512, 512]), (19, 10): ([10, 9], [1024, 512]), (20, 10): ([10, 10], [1024, 1024]),
    (19, 11): ([10, 9], [1024, 512]), (20, 11): ([10, 10], [1024, 1024]), (21, 11): ([11, 10], [512, 1024]), (22, 11): ([11, 11], [512, 512]),
}


@pytest.mark.parametrize("log_n,max_radix", sorted(PLANS))
def test_plans_the_gpu_tests_rely_on(log_n, max_radix):
    p = B.ntt_plan_info(log_n, max_radix)
    radices, threads = PLANS[(log_n, max_radix)]
    assert (p["log_radix"], p["threads"]) == (radices, threads)
    assert p["log_tile"] == ([log_n] if len(radices) == 1 else [{256: 10, 512: 11, 1024: 12}[t] for t in threads])
