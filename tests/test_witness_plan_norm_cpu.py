"""The RECIP and ISQRT record kinds on the host: the interpreter (witness_plan.run_plan_host) against the closed form of
tests/witness_synth_norm.py, both validators on every plan and on the plans they must refuse, with the same words, the upload refusing
those before a device is asked for; NormCircuit -- softmax and layer norm -- recorded to the cells of the host layout, with one RECIP
record for all softmax rows; kinds 16 and 23 refused as unknown; and the MLP recorder refusing the new ops by name."""
import ctypes as C

import numpy as np
import pytest

import witness_synth as S
import witness_synth_norm as T


def _check(L, plan):
    blob = plan.to_bytes()
    return L.ezkl_prover_witness_plan_check(blob, C.c_size_t(len(blob)))


@pytest.fixture(scope="module")
def parser():
    from ezkl_amd import native
    return native.load()


def _assert_columns(plan, cols, want):
    for c in range(plan.n_advice):
        assert cols[c] == want[c], "column %d differs on rows %s" % (c, [r for r in range(1 << plan.k) if cols[c][r] != want[c][r]][:8])


@pytest.mark.parametrize("name", list(T.CASES))
def test_the_host_interpreter_equals_the_closed_form(parser, name):
    from ezkl_amd import witness_plan as WP
    kind = WP.RECIP if name.startswith("recip") else WP.ISQRT
    for seed in (1, 2):
        case = T.CASES[name](seed)
        plan = case.plan.validate()
        assert _check(parser, plan) == 0, parser.ezkl_prover_last_error().decode()
        assert WP.WitnessPlan.from_bytes(plan.to_bytes()) == plan == T.CASES[name](seed).plan, "seeded: the same bytes again"
        assert len(case.expect) == plan.n_cells and plan.records[:, 0].tolist() == [WP.INPUT, kind] and not case.refused
        cols, outs = WP.run_plan_host(plan, case.x)
        _assert_columns(plan, cols, case.columns())
        assert outs == case.outputs()


def test_the_cases_plant_what_they_claim():
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    assert (WP.RECIP, WP.ISQRT, WP.VERSION) == (24, 25, 1) and (WP.RECIP_ERROR, WP.SQRT_ERROR) == (EL.RECIP_ERROR, EL.SQRT_ERROR)
    assert [WP.kind_name(kd) for kd in (WP.ARGSORT, 23, WP.RECIP, WP.ISQRT, 26, 16)] == ["argsort", "?", "recip", "sqrt", "?", "?"]
    assert T.COUNTS == [1, 63, 64, 65, 255, 256, 257] and T.RECIP_SCALES == [1, 1 << 21, (1 << 62) - 1] and T.SQRT_SCALES == [1, 128, (1 << 31) - 1]
    assert [T.recip_expected(x, 1) for x in (1, 2, 3, -1, -2, -3)] == [1, 0, 0, -1, -1, 0], "the ties +-2S: towards zero above, away from it below"
    assert [T.sqrt_expected(t) for t in (1, 2, 3, 6, 7, (1 << 62) - 1)] == [1, 1, 2, 2, 3, 1 << 31]
    for scale in T.RECIP_SCALES:
        vals = [S.signed(v % S.R) for v in T.CASES["recip-n65-S%d" % scale](1).x]
        assert set(T.recip_values(scale)) <= set(vals) and {0, scale, -scale, S.FIT - 1, -(S.FIT - 1)} <= set(vals)
        assert scale > 1 << 60 or {2 * scale, -2 * scale, 2 * scale - 1, 2 * scale + 1, -(2 * scale + 1)} <= set(vals)
    for scale in T.SQRT_SCALES:
        vals = T.CASES["sqrt-n257-scale%d" % scale](2).x
        assert set(T.sqrt_values(scale)) <= set(vals) and (S.FIT - 1) // scale in vals and min(vals) < 0 and max(v * scale for v in vals) < S.FIT
        assert T.too_large(scale) * scale >= S.FIT > (T.too_large(scale) - 1) * scale
    top = (1 << 31) - 1
    assert {0, 1, 2, 3, top * top, top * top + top, top * top + top + 1, 65535 * 65535 + 65535, S.FIT - 1} <= set(T.sqrt_values(1))
    small = T.small_plan()
    assert [S.signed(v) for v in small.columns()[1][:4]] == [99, 1, -2, 0] and small.columns()[2][:4] == [0, 6, 4, 0]      # S = 6 over 4, -4, 12: three ties


@pytest.mark.parametrize("kind,scale", [("recip", s) for s in T.RECIP_SCALES] + [("sqrt", s) for s in T.SQRT_SCALES])
def test_an_operand_beyond_the_range_is_named_with_the_smallest_element(parser, kind, scale):
    from ezkl_amd import witness_plan as WP
    kd, words = (WP.RECIP, WP.RECIP_ERROR) if kind == "recip" else (WP.ISQRT, WP.SQRT_ERROR)
    good, bad = T.failing_case(kd, scale, False, seed=3), T.failing_case(kd, scale, True, seed=4)
    assert _check(parser, bad.plan.validate()) == 0 and bad.plan == good.plan
    cols, outs = WP.run_plan_host(good.plan, good.x)
    _assert_columns(good.plan, cols, good.columns())
    assert outs == good.outputs() and not good.refused
    assert bad.refused == [(1, e) for e in T.BAD_AT] and len(bad.unwritten) == 2 and all(bad.expect[c] == 0 for c in bad.unwritten)
    with pytest.raises(AssertionError, match=r"%s \(%s record 1, element %d\)" % (words, kind, T.BAD_AT[0])):
        WP.run_plan_host(bad.plan, bad.x)


def test_both_validators_refuse_each_bad_shape_with_the_same_words(parser):
    from ezkl_amd import lib, witness_plan as WP
    H = lib.load()
    good = T.small_plan()
    assert _check(parser, good.plan.validate()) == 0
    cols, outs = WP.run_plan_host(good.plan, good.x)
    assert cols == good.columns() and outs == good.outputs() == [99, 0, 6, 4]
    seen = set()
    for words, rec, plan in T.bad_plans():
        name = WP.kind_name(plan.records[rec, 0])
        assert name in ("recip", "sqrt")
        with pytest.raises(WP.PlanError) as e:
            WP.validate(plan)
        assert str(e.value) == "witness plan: record %d (%s): %s" % (rec, name, words)
        with pytest.raises(WP.PlanError, match=words.replace("[", r"\[").replace(")", r"\)").replace("^", r"\^")):
            WP.run_plan_host(plan, good.x)
        assert _check(parser, plan) == -3, words
        assert parser.ezkl_prover_last_error().decode().endswith(str(e.value)), (words, parser.ezkl_prover_last_error())
        blob, h = plan.to_bytes(), C.c_void_p()
        assert H.ezkl_hip_witness_plan_upload(blob, C.c_size_t(len(blob)), C.byref(h)) == -3 and not h.value      # before a device is asked for
        assert H.ezkl_hip_witness_last_error().decode() == str(e.value)
        seen.add(words)
    assert seen == {"reciprocal scale outside [1, 2^62)", "zero-inverse index past the constants", "zero square-root scale",
                    "a square-root record with a second parameter", "a cell is read before an earlier record has written it", "cell index out of range",
                    "a cell is written twice"}


def test_kinds_16_and_23_and_the_end_marker_are_refused_as_unknown(parser):
    from ezkl_amd import witness_plan as WP
    plan = T.small_plan().plan
    for rec in (1, 2):
        for kind in (16, 23, 26, 0xFFFFFFFF):
            q = T._tampered(plan)
            q.records[rec, 0] = kind
            with pytest.raises(WP.PlanError, match=r"record %d: unknown kind %d" % (rec, kind)):
                WP.validate(q)
            assert _check(parser, q) == -3 and parser.ezkl_prover_last_error().decode().endswith("witness plan: record %d (?): unknown kind" % rec)


# ---- recording: NormCircuit ---------------------------------------------------------------------------------------------------------------------
def _circuit(variant, rows=2, length=4, **kw):
    from ezkl_amd import ezkl_layout as EL
    return EL.NormCircuit(9, 2, 3000, rows, length, layer_norm=(variant == "layer_norm"), **kw)


def _inputs(n, seed):
    return np.random.default_rng(seed).integers(-12, 13, n).tolist()


@pytest.mark.parametrize("variant", ["softmax", "layer_norm"])
def test_the_norm_circuit_records_to_the_cells_of_the_host_engine(parser, variant):
    from ezkl_amd import witness_plan as WP
    c = _circuit(variant)
    plan = WP.record_plan(c).validate()
    assert _check(parser, plan) == 0, parser.ezkl_prover_last_error().decode()
    assert WP.WitnessPlan.from_bytes(plan.to_bytes()) == plan and WP.peek(plan.to_bytes())["k"] == 9
    kinds = plan.records[:, 0].tolist()
    recips = [r for r in plan.records.tolist() if r[0] == WP.RECIP]
    roots = [r for r in plan.records.tolist() if r[0] == WP.ISQRT]
    S_, zi = 8 * 64, 8192
    assert len(recips) == 1 and recips[0][1:4] == [2, S_, 0] and plan.consts[recips[0][6]] == zi, "one RECIP record for both rows: one dependence level"
    if variant == "softmax":
        assert not roots and kinds.count(WP.SORT) == 1 and kinds.count(WP.TABLE) == 1 and kinds.count(WP.SUMACC) == 1
    else:
        # `abs` places the claimed root twice (its decomposition, then its product with the sign), as `sqrt` of layouts.rs does: one level
        assert len(roots) == 1 and roots[0][1:4] == [4, 8, 0] and WP.SORT not in kinds and WP.TABLE not in kinds
    for seed in (1, 2, 3):
        x = _inputs(8, seed)
        adv, inst = _circuit(variant).witness(x)
        cols, outs = WP.run_plan_host(plan, x)
        for i, (got, want) in enumerate(zip(cols, adv)):
            assert got == want, "advice column %d differs on rows %s" % (i, [r for r in range(1 << 9) if got[r] != want[r]][:8])
        assert outs == inst[0] and len(cols) == len(adv)


def test_a_zero_and_a_tie_replay_from_the_plan():
    """the constant row (root 0 -> zero_inverse) and the softmax tie (exp-sum = 2S) of tests/test_norm_layout_cpu.py, from their plans"""
    from ezkl_amd import witness_plan as WP
    from test_norm_layout_cpu import TIE
    for c, x in ((_circuit("layer_norm"), [7, 7, 7, 7, 3, -4, 9, 0]), (_circuit("softmax", **TIE), [0, -200, 0, -200, 5, 5, -200, -200])):
        cols, outs = WP.run_plan_host(WP.record_plan(c).validate(), x)
        assert (cols, [outs]) == c.witness(x)


def test_more_rows_still_share_their_records():
    from ezkl_amd import witness_plan as WP
    two, five = (WP.record_plan(_circuit("softmax", rows=r)) for r in (2, 5))
    assert two.n_records == five.n_records and five.n_cells > 2 * two.n_cells
    assert [r[1] for r in five.records.tolist() if r[0] == WP.RECIP] == [5]
    x = _inputs(20, 9)
    c = _circuit("softmax", rows=5)
    assert WP.run_plan_host(five.validate(), x) == (c.witness(x)[0], c.outputs)


def test_the_recorders_keep_their_refusals():
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    mlp_reg = WP.RecordingRegion(EL.MlpCircuit(8, 2, [], [], 128, 2, n_inputs=3, relu_first=True).gc)
    for op, args in (("recip", ([], 1, 1, 0.5)), ("sqrt", ([], 1)), ("rsqrt", ([], 1, 1, 0.5)), ("softmax", ([], 1, 1, 0.5)), ("max", ([],))):
        with pytest.raises(WP.PlanError, match="witness plans do not cover `%s`" % op):
            getattr(mlp_reg, op)(*args)
    reg = WP.LookupRecordingRegion(_circuit("layer_norm").gc)
    reg.decomp = (128, 2)
    with pytest.raises(WP.PlanError, match="does not cover"):
        reg.recip([EL.Val(WP._Input(0))], 8, 64, 1.0 / 128)             # a reciprocal of a value that is no assigned cell
    cell = reg.assign(reg.inputs[0], [EL.Val(WP._Input(0))])
    with pytest.raises(WP.PlanError, match=r"a reciprocal at a scale outside \[1, 2\^62\)"):
        reg.recip(cell, 1 << 31, 1 << 31, 1.0)
    with pytest.raises(WP.PlanError, match=r"a square root at a scale outside \[1, 2\^32\)"):
        reg.sqrt(cell, 1 << 32)
