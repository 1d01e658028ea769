"""GPU parity of the MSM under its PER-CALL tuning variables (msm.hip: msm_tuning reads EZKL_MSM_L and EZKL_MSM_E at every call, and
msm_plan.hpp sizes the lanes, the reduce stages and the scratch regions from them): one MSM per setting, compared byte for byte with
oracle.binding.msm.  EZKL_MSM_L = 8 / 64 are a lane length below and above what the plan picks at these sizes, EZKL_MSM_E = 1 / 1024 the two
ends of the first reduce stage (no serial elements per lane: n_partA = every bucket; all of them: one group); a value outside the accepted
range (0, and 3 for E: not a power of two) must leave the default in force.  The variables that are read once per process are not tested.
Sizes: 1025 (W = 24, three tiles, no in-partition bucket bits: the small-MSM field split) and 4097 (W = 20, seven tiles, LB = 2);
tests/cpp/test_msm_plan.cpp holds the plan itself to its invariants at every size, without a device."""
import numpy as np
import pytest
from conftest import SEED
from oracle import binding as ob
from test_gpu_msm_groups import _column

pytestmark = pytest.mark.gpu

SIZES = (1025, 4097)
KINDS = ("uniform", "witness20")
SETTINGS = [("EZKL_MSM_L", v) for v in ("8", "64", "0")] + [("EZKL_MSM_E", v) for v in ("1", "1024", "0", "3")]

_CASES = {}


def _case(n, kind):
    """(bases, device column, oracle result) of one kind at one size: made once, shared by every setting, never modified"""
    from ezkl_amd import backend as B
    if (n, kind) not in _CASES:
        pts = ob.gen_bases(SEED + 31, n)
        col = _column(kind, np.random.default_rng(3000 + n + KINDS.index(kind)), n)
        _CASES[(n, kind)] = (B.Bases(pts), B.DeviceBuffer.from_numpy(col), ob.msm(col, pts))
    return _CASES[(n, kind)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("var,value", SETTINGS)
def test_per_call_tuning_matches_the_oracle(hip, monkeypatch, var, value, n, kind):
    from ezkl_amd import backend as B
    bases, dev, want = _case(n, kind)
    monkeypatch.setenv(var, value)
    assert (B.msm_g1_dev(bases, dev.ptr, n) == want).all(), (var, value, n, kind)
