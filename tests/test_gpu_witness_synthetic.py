"""The witness kernels (csrc/witness.hip) on the synthetic plans of tests/witness_synth.py: every device column byte-equal to the closed
form -- not to the host interpreter, which tests/test_witness_synthetic_cpu.py holds to the same closed form -- with full-range field
elements, 64-bit integers, decompositions up to 2^62, every block edge of the element-wise kernel and every chunk edge of the dot scan;
every case twice into the same columns; the exact failure count, the first failing (record, element) and untouched refused cells;
and the order of three phases, a failed middle phase included."""
import re

import pytest

import witness_synth as S

pytestmark = pytest.mark.gpu
SEEDS = (1, 2)


def _message(plan, refused):
    from ezkl_amd import witness_plan as WP
    ri, el = refused[0]
    kind = int(plan.records[ri, 0])
    text = WP.LOOKUP_ERROR if kind in (WP.TABLE, WP.TBLIDX) else WP.DIV_ERROR if kind == WP.DIVC else WP.RANGE_ERROR
    return re.escape("%s (%s record %d, element %d; %d cells in all)" % (text, WP.KIND_NAMES[kind], ri, el, len(refused)))


def _assert_columns(cols, case, only=None):
    from ezkl_amd import ezkl_layout as EL
    k = case.plan.k
    got = {}
    for c, want in enumerate(EL.cols_to_mont(case.columns())):
        if only is not None and c not in only:
            continue
        got[c] = cols[c].to_numpy(shape=(1 << k, 4))
        assert got[c].tobytes() == want.tobytes(), "column %d differs on rows %s" % (c, (got[c] != want).any(1).nonzero()[0][:8].tolist())
    for cell in case.refused_cells:
        assert not got[cell >> k][cell & ((1 << k) - 1)].any(), "a refused lane wrote cell %d" % cell
    for cell, total in case.dot_totals:                              # the last live cell of a dot: the whole sum of products
        if cell >> k in got:
            assert got[cell >> k][cell & ((1 << k) - 1)].tobytes() == EL.ints_to_mont([total]).tobytes()


def _run(B, dev, cols, case):
    """one single-phase run into `cols`: a passing case, or one whose refused lanes are known"""
    plan = case.plan
    if case.refused:
        with pytest.raises(B.WitnessError, match=_message(plan, case.refused)):
            dev.run(case.x, columns=cols)
        assert dev.last["failed"] == len(case.refused) and dev.last["first"] == case.refused[0]
    else:
        _, outs = dev.run(case.x, columns=cols)
        assert outs == case.outputs() and dev.last["failed"] == 0
    assert dev.last["cells_written"] == plan.n_cells - len(case.refused)
    _assert_columns(cols, case)


@pytest.mark.parametrize("name", list(S.CASES))
def test_device_columns_equal_the_closed_form(hip, name):
    from ezkl_amd import backend as B
    cols, devs = None, []
    try:
        for seed in SEEDS:                                           # other values into the columns the first run left dirty
            case = S.CASES[name](seed)
            devs.append(B.WitnessPlan(case.plan.to_bytes()))
            cols = cols or devs[-1].alloc_columns()
            _run(B, devs[-1], cols, case)
    finally:
        for c in cols or []:
            c.free()
        for dev in devs:
            dev.free()


@pytest.mark.parametrize("variant", [0, 1])
def test_failures_are_counted_exactly_and_refused_cells_stay_zero(hip, variant):
    from ezkl_amd import backend as B, witness_plan as WP
    bad = S.accounting_case(variant, True, seed=7)
    dev = B.WitnessPlan(bad.plan.to_bytes())
    cols = dev.alloc_columns()
    try:
        _run(B, dev, cols, S.accounting_case(variant, False, seed=6))      # every cell non-zero-filled by a run before the failing one
        assert len(bad.refused) == 10 and bad.refused[0] == ((1, 3), (1, 64))[variant]
        _run(B, dev, cols, bad)
        with pytest.raises(AssertionError, match=r"value exceeds the decomposition range \(decompose record %d, element %d\)" % bad.refused[0]):
            WP.run_plan_host(bad.plan, bad.x)
        _run(B, dev, cols, S.accounting_case(variant, False, seed=8))      # the next valid run, the same columns
    finally:
        for c in cols:
            c.free()
        dev.free()


def test_three_phases_and_a_failed_middle_phase(hip):
    """assertion 3 (phase 2 refused after a phase 1 that failed on columns an earlier phase 1 had finished) needs done_phase lowered when a
    phase STARTS; before that fix the phase-2 run was accepted and read the half-written columns"""
    from ezkl_amd import backend as B
    R = S.R
    ok, big = S.three_phase_case(1, 3), S.large_challenge(3)
    bad, other = S.three_phase_case(big, 3), S.three_phase_case(1, 4)
    plan = ok.plan
    assert plan == other.plan and (bad.plan.records == plan.records[:3]).all() and bad.x == ok.x and bad.refused and not ok.refused
    dev = B.WitnessPlan(plan.to_bytes())
    cols = dev.alloc_columns()

    def phases(case, which):
        written, outs = 0, None
        for ph in which:
            _, outs = dev.run(case.x if ph == 0 else None, columns=cols, phase=ph, challenges=case.challenges)
            assert dev.last["failed"] == 0
            written += dev.last["cells_written"]
        return written, outs

    def refused_phase_2():
        with pytest.raises(ValueError, match="phase 2 before phase 1") as e:
            dev.run(None, columns=cols, phase=2, challenges=[1])
        assert not isinstance(e.value, B.WitnessError) and dev.last["launches"] == 0 and dev.last["cells_written"] == 0

    try:
        assert (dev.n_phases, dev.n_challenges, dev.column_phase) == (3, 1, [0, 1, 1, 2])
        written, outs = phases(ok, (0, 1, 2))                                        # 1
        assert written == plan.n_cells and outs == ok.outputs()
        _assert_columns(cols, ok)
        with pytest.raises(B.WitnessError, match=_message(plan, bad.refused)):       # 2
            dev.run(None, columns=cols, phase=1, challenges=[big])
        assert bad.refused[0][0] == 2 and dev.last["failed"] == len(bad.refused) and dev.last["first"] == bad.refused[0]
        m = S.PHASED_SCANS * S.PHASED_STEPS
        assert dev.last["cells_written"] == 4 * m - len(bad.refused)
        _assert_columns(cols, bad, only=(0, 1, 2))
        refused_phase_2()                                                            # 3
        written, outs = phases(ok, (1, 2))                                           # 4
        assert outs == ok.outputs()
        _assert_columns(cols, ok)
        phases(other, (0,))                                                          # 5
        refused_phase_2()
        flipped = S.three_phase_case(R - 1, 4)                                       # 6: alternating sums, in range
        assert not flipped.refused
        phases(flipped, (1,))
        _assert_columns(cols, flipped, only=(0, 1, 2))
        written, outs = phases(other, (1, 2))
        assert outs == other.outputs()
        _assert_columns(cols, other)
    finally:
        for c in cols:
            c.free()
        dev.free()
