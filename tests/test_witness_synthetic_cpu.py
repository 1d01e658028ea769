"""The host interpreter (witness_plan.run_plan_host) against the closed-form expectations of tests/witness_synth.py: synthetic plans with
full-range field elements, 64-bit integers, decompositions up to 2^62, every block and chunk edge of the device kernels.  Every plan
passes witness_plan.validate and the C++ parser; a lane a kind must refuse is named by the interpreter with the record and element the
closed form names; the two decomposition shapes at 2^62 are refused by both validators and by the upload."""
import ctypes as C

import pytest

import witness_synth as S


def _check(L, plan):
    blob = plan.to_bytes()
    return L.ezkl_prover_witness_plan_check(blob, C.c_size_t(len(blob)))


@pytest.fixture(scope="module")
def parser():
    from ezkl_amd import native
    return native.load()


@pytest.mark.parametrize("name", list(S.CASES))
def test_the_host_interpreter_equals_the_closed_form(parser, name):
    from ezkl_amd import witness_plan as WP
    for seed in (1, 2):
        case = S.CASES[name](seed)
        plan = case.plan.validate()
        assert _check(parser, plan) == 0, parser.ezkl_prover_last_error().decode()
        assert WP.WitnessPlan.from_bytes(plan.to_bytes()) == plan == S.CASES[name](seed).plan, "seeded: the same bytes again"
        assert len(case.expect) == plan.n_cells
        if case.refused:
            ri, el = case.refused[0]
            with pytest.raises(AssertionError, match=r"\(%s record %d, element %d\)" % (WP.KIND_NAMES[plan.records[ri, 0]], ri, el)):
                WP.run_plan_host(plan, case.x)
            continue
        cols, outs = WP.run_plan_host(plan, case.x)
        want = case.columns()
        for c in range(plan.n_advice):
            assert cols[c] == want[c], "column %d differs on rows %s" % (c, [r for r in range(1 << plan.k) if cols[c][r] != want[c][r]][:8])
        assert outs == case.outputs()
        for cell, total in case.dot_totals:                           # the last live cell of a dot: the whole sum of products
            assert cols[cell >> plan.k][cell & ((1 << plan.k) - 1)] == total


def test_the_cases_plant_what_they_claim():
    """the value lists reach the edges the case names promise (a builder that quietly dropped them would leave the tests green)"""
    R, H = S.R, S.HALF
    ops = S.field_operands(1)
    assert {0, 1, R - 1, H - 1, H, H + 1, (1 << 255) % R} <= set(ops) and all(1 << (32 * i) in ops for i in range(1, 8)) and len(ops) == 53
    assert all(0 <= v < R for v in ops) and ops != S.field_operands(2)
    assert [S.signed(v) for v in (H - 1, H, H + 1, R - 1, 0)] == [H - 1, -(H + 1), -H, -1, 0]
    case = S.CASES["elem-count513-permuted"](1)
    n, corners = 1 << case.plan.k, set()
    for c in case.expect:
        if c & (n - 1) in (0, n - 1) and c >> case.plan.k in (0, case.plan.n_advice - 1):
            corners.add(c)
    assert len(corners) == 4, "row 0 and row 2^k - 1 of the first and the last column are destinations"
    assert any(a + b >= R for a, b in S.WRAP_PAIRS) and any(a < b for a, b in S.WRAP_PAIRS) and (R - 1, R - 1) in S.WRAP_PAIRS
    assert {S.INT64_MIN, S.INT64_MAX, 1 << 62, -(1 << 62), 0, 1, -1} <= set(case.x)
    wide = S.CASES["elem-advice64-k4"](1).plan
    assert wide.n_advice == 64 and {0, 31, 63} == {int(c) >> 4 for c in S.CASES["elem-advice64-k4"](1).expect}
    assert len(S.too_large()) == 19 and all(abs(S.signed(v)) >= 1 << 62 for v in S.too_large())
    for name in S.REFUSE_KINDS:
        assert len(S.CASES["refuse-" + name](1).refused) == 19 and len(S.CASES["refuse-" + name](1).expect) == 2 * 22
    ragged = S.CASES["dot-ragged-1-5-16-17-33"](1).plan
    assert ragged.records[1].tolist()[:4] == [S.WP.DOT, 5, 2, 33] and ragged.n_cells == 53 + 72


@pytest.mark.parametrize("base,legs", [(2, 62), (1 << 31, 2)])
def test_a_decomposition_at_two_to_the_62_is_refused_by_both_validators_and_the_upload(parser, base, legs):
    from ezkl_amd import lib, witness_plan as WP
    b = S.Builder(4, 2)
    src = b.input(b.rows(0, range(3)), [0, 1, -1])
    b.records.append([WP.HINT, 3, base, legs, b._push(b.rows(1, range(3))), b._push(src.idx), b._push([S.NONE, 0, legs - 1]), 0])
    b.n_cells += 3
    plan = b.plan()
    assert base ** legs == 1 << 62
    with pytest.raises(WP.PlanError, match="bad decomposition"):
        WP.validate(plan)
    assert _check(parser, plan) == -3 and "bad decomposition" in parser.ezkl_prover_last_error().decode()
    H, h, blob = lib.load(), C.c_void_p(), plan.to_bytes()
    assert H.ezkl_hip_witness_plan_upload(blob, C.c_size_t(len(blob)), C.byref(h)) == -3 and not h.value       # before a device is asked for
    assert "bad decomposition" in H.ezkl_hip_witness_last_error().decode()
    plan.records = plan.records.copy()                              # one leg less: the largest shape that is taken
    plan.records[1, 3] = legs - 1
    plan.pool = plan.pool.copy()
    plan.pool[-1] = legs - 2
    WP.validate(plan)
    assert _check(parser, plan) == 0


@pytest.mark.parametrize("variant", [0, 1])
def test_failure_accounting_on_the_host(parser, variant):
    from ezkl_amd import witness_plan as WP
    bad, good = S.accounting_case(variant, True), S.accounting_case(variant, False)
    assert bad.plan == good.plan and _check(parser, bad.plan.validate()) == 0
    assert len(bad.refused) == 5 + 2 + 3 and bad.refused[0] == ((1, 3), (1, 64))[variant] and not good.refused
    with pytest.raises(AssertionError, match=r"value exceeds the decomposition range \(decompose record %d, element %d\)" % bad.refused[0]):
        WP.run_plan_host(bad.plan, bad.x)
    cols, outs = WP.run_plan_host(good.plan, good.x)
    assert cols == good.columns() and outs == good.outputs()


def test_three_phases_on_the_host(parser):
    from ezkl_amd import witness_plan as WP
    ok = S.three_phase_case(1, 3)
    plan = ok.plan.validate()
    assert _check(parser, plan) == 0 and WP.column_phases(plan) == [0, 1, 1, 2] and plan.n_phases == 3 == WP.MAX_PHASES
    assert not ok.refused and len(ok.expect) == plan.n_cells
    cols, outs = WP.run_plan_host(plan, ok.x, challenges=[1])
    assert cols == ok.columns() and outs == ok.outputs()
    for cell, total in ok.dot_totals:
        assert cols[3][cell & 511] == total
    for c in (S.large_challenge(3), S.R - 1):
        case = S.three_phase_case(c, 3)
        if c == S.R - 1:                                            # alternating sums of small inputs: still in range, still the closed form
            assert not case.refused and case.plan == plan
            assert WP.run_plan_host(plan, case.x, challenges=[c])[0] == case.columns()
            continue
        ri, el = case.refused[0]
        assert ri == 2 and len(case.refused) > 300 and case.x == ok.x
        with pytest.raises(AssertionError, match=r"value exceeds the decomposition range \(decompose record 2, element %d\)" % el):
            WP.run_plan_host(plan, case.x, challenges=[c])
