"""The SORT and ARGSORT record kinds on the host: the interpreter (witness_plan.run_plan_host) against the closed form of
tests/witness_synth_sort.py, both validators on every plan and on the plans they must refuse, with the same words, the upload refusing
those before a device is asked for; SortTopkCircuit recorded to the cells of the host layout; and the blobs of the circuit families that
were recorded before: their bytes have not moved."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import witness_synth as S
import witness_synth_sort as T

MODES = ["unsorted", "smallest_index_first", "largest_index_first"]


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
    for seed in (1, 2):
        case = T.CASES[name](seed)
        plan = case.plan.validate()
        assert _check(parser, plan) == 0, parser.ezkl_prover_last_error().decode()
        assert WP.WitnessPlan.from_bytes(plan.to_bytes()) == plan == T.CASES[name](seed).plan, "seeded: the same bytes again"
        assert len(case.expect) == plan.n_cells and plan.records[:, 0].tolist() == [WP.INPUT, WP.SORT, WP.ARGSORT]
        cols, outs = WP.run_plan_host(plan, case.x)
        _assert_columns(plan, cols, case.columns())
        assert outs == case.outputs()


def test_the_cases_plant_what_they_claim():
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    assert (WP.SORT, WP.ARGSORT, WP.VERSION) == (21, 22, 1) and WP.SORT_TILE == 2048 and WP.SORT_ERROR == EL.SORT_ERROR == "sort key beyond 62 bits"
    assert [WP.kind_name(kd) for kd in (WP.CLAMP, WP.SORT, WP.ARGSORT, 23, 16)] == ["clamp", "sort", "argsort", "?", "?"]
    assert T.LENGTHS == [1, 2, 3, 63, 64, 65, 2047, 2048, 2049, 4101]
    assert T.ranks([5, -2, 5, 0], 0) == [2, 0, 3, 1] and T.ranks([5, -2, 5, 0], 1) == [3, 0, 2, 1]
    edges = T.CASES["sort-n65-mode1"](1)
    vals = [S.signed(v % S.R) for v in edges.x]
    assert {S.FIT - 1, -(S.FIT - 1), 0, -1} <= set(vals[4 * 65:5 * 65]) and len(set(vals[:65])) == 1 and len(set(vals[65:130])) == 2
    assert vals[130:195] == sorted(vals[130:195]) and vals[195:260] == sorted(vals[195:260], reverse=True)
    many = T.CASES["sort-300x5-mode0"](1).plan
    assert many.records[1].tolist()[:4] == [WP.SORT, 1500, 5, 0] and many.records[2].tolist()[:4] == [WP.ARGSORT, 1500, 5, 0]
    assert T.CASES["sort-9x100-mode1"](1).plan.records[2].tolist()[:4] == [WP.ARGSORT, 900, 100, 1]
    small = T.small_plan()
    n = 1 << small.plan.k
    assert [S.signed(v) for v in small.columns()[1][:8]] == [-2, 0, 5, 5, -7, 3, 3, 9] and small.columns()[2][:8] == [1, 3, 2, 0, 2, 1, 0, 3] and n == 16


@pytest.mark.parametrize("n", [100, T.TILE + 1])
def test_a_key_beyond_62_bits_is_named_with_the_smallest_record_and_element(parser, n):
    from ezkl_amd import witness_plan as WP
    good, bad = T.failing_case(n, False, seed=3), T.failing_case(n, True, seed=4)
    assert _check(parser, bad.plan.validate()) == 0 and bad.plan == T.failing_case(n, False, seed=5).plan
    cols, outs = WP.run_plan_host(good.plan, good.x)
    _assert_columns(good.plan, cols, good.columns())
    assert outs == good.outputs() and not good.refused and not good.unwritten
    sort_ri, arg_ri = [ri for ri, r in enumerate(bad.plan.records.tolist()) if r[0] in (WP.SORT, WP.ARGSORT)]
    assert bad.refused == [(ri, n + e) for ri in (sort_ri, arg_ri) for e in T.BAD_AT] and len(bad.unwritten) == 2 * n
    assert all(bad.expect[c] == 0 for c in bad.unwritten) and sum(1 for v in bad.expect.values() if v) > 2 * n, "the neighbour segments are written"
    with pytest.raises(AssertionError, match=r"sort key beyond 62 bits \(sort record %d, element %d\)" % (sort_ri, n + T.BAD_AT[0])):
        WP.run_plan_host(bad.plan, bad.x)


def test_both_validators_refuse_each_bad_shape_with_the_same_words(parser):
    from ezkl_amd import lib, witness_plan as WP
    H = lib.load()
    good = T.small_plan()
    assert _check(parser, good.plan.validate()) == 0
    cols, outs = WP.run_plan_host(good.plan, good.x)
    assert cols == good.columns() and outs == good.outputs() == [(-2) % S.R, 1]
    seen = set()
    for words, rec, plan in T.bad_plans():
        name = WP.kind_name(plan.records[rec, 0])
        assert name in ("sort", "argsort")
        with pytest.raises(WP.PlanError) as e:
            WP.validate(plan)
        assert str(e.value) == "witness plan: record %d (%s): %s" % (rec, name, words)
        with pytest.raises(WP.PlanError, match=words):
            WP.run_plan_host(plan, good.x)
        assert _check(parser, plan) == -3, words
        assert parser.ezkl_prover_last_error().decode().endswith(str(e.value)), (words, parser.ezkl_prover_last_error())
        blob, h = plan.to_bytes(), C.c_void_p()
        assert H.ezkl_hip_witness_plan_upload(blob, C.c_size_t(len(blob)), C.byref(h)) == -3 and not h.value      # before a device is asked for
        assert H.ezkl_hip_witness_last_error().decode() == str(e.value)
        seen.add(words)
    assert seen == {"bad sort shape", "a cell is read before an earlier record has written it", "cell index out of range", "a cell is written twice"}


def test_the_blobs_of_the_earlier_families_keep_their_bytes():
    """the kinds are appended and the version word stays 1: the circuits recorded before record to the bytes the existing tests pin (their
    digests, taken on the commits those files name) and to no record of a new kind -- the surrogate, whose shuffle goes through
    `_lookup_any`, among them"""
    from ezkl_amd import witness_plan as WP
    import test_witness_plan_lookup_cpu as TL
    import test_witness_plan_phases_cpu as TP
    from test_witness_plan_cpu import _mlp
    plans = {TL.MLP_PINS["mlp_k9_w2_3_blocks"][1]: WP.record_plan(_mlp(9, 2)[0]),
             TL.CONV_PINS["conv_k10_w2"][1]: WP.record_plan(TL.CASES["conv_k10_w2"]()[0]),
             TP.PINS[(6, 3)][0]: TP.recorded(6, 3)[4]}
    for sha, plan in plans.items():
        assert hashlib.sha256(plan.to_bytes()).hexdigest() == sha and len(sha) == 64
        assert int(plan.records[:, 0].max()) <= WP.DIVC and WP.peek(plan.to_bytes())["k"] == plan.k


# ---- recording: SortTopkCircuit ---------------------------------------------------------------------------------------------------------------
def _circuit(k, length, mode, w=2, k_top=None, largest=True):
    from ezkl_amd import ezkl_layout as EL
    return EL.SortTopkCircuit(k, w, 3000, length, min(3, length) if k_top is None else k_top, largest, mode, 16, 2)


def _inputs(length, seed):
    """values in [-100, 100], one of them twice"""
    x = np.random.default_rng(seed).integers(-100, 101, length).tolist()
    x[-1] = x[0]
    return x


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("length", [2, 3, 8, 13])
def test_sort_and_topk_record_to_the_cells_of_the_host_engine(parser, length, mode):
    from ezkl_amd import witness_plan as WP
    c = _circuit(9, length, mode)
    plan = WP.record_plan(c).validate()
    assert _check(parser, plan) == 0, parser.ezkl_prover_last_error().decode()
    kinds = plan.records[:, 0].tolist()
    assert kinds.count(WP.SORT) >= 1 and kinds.count(WP.ARGSORT) >= 1
    sorts = [r for r in plan.records.tolist() if r[0] in (WP.SORT, WP.ARGSORT)]
    assert all(r[2] == length and r[1] % length == 0 for r in sorts) and sum(r[1] for r in sorts) == 4 * length, "the top-k's sort and the full one"
    assert {r[3] for r in sorts} == ({0, 1} if mode == "largest_index_first" else {0})
    for seed in (1, 2):
        x = _inputs(length, 10 * length + seed)
        adv, inst = c.witness(x)
        cols, outs = WP.run_plan_host(plan, x)
        for i, (got, want) in enumerate(zip(cols, adv)):
            assert got == want, "advice column %d differs on rows %s" % (i, [r for r in range(1 << 9) if got[r] != want[r]][:8])
        assert outs == inst[0] and len(cols) == len(adv)
        assert [S.signed(v) for v in outs] == sorted(x, reverse=True)[:min(3, length)] + sorted(x)


def test_a_sort_of_one_element_records_no_sort():
    from ezkl_amd import witness_plan as WP
    c = _circuit(9, 1, "smallest_index_first")
    plan = WP.record_plan(c).validate()
    assert plan.records[:, 0].tolist() == [WP.INPUT] and plan.n_cells == 1
    cols, outs = WP.run_plan_host(plan, [-5])
    assert (cols, [outs]) == c.witness([-5]) and outs == [(-5) % S.R] * 2


def test_two_rows_of_a_topk_axes_land_in_one_record_with_two_segments():
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    from test_sort_layout_cpu import TwoRowsCircuit
    c = TwoRowsCircuit(3, 2)
    plan = WP.record_plan(c).validate()
    sorts = [r for r in plan.records.tolist() if r[0] in (WP.SORT, WP.ARGSORT)]
    assert [r[:4] for r in sorts] == [[WP.SORT, 6, 3, 0], [WP.ARGSORT, 6, 3, 0]]
    x = [2, 15, 2, 1, 1, 0]                                             # the doc example of the reference's topk_axes
    cols, outs = WP.run_plan_host(plan, x)
    assert outs == [15, 2, 1, 1]
    reg = EL.BaseRegion(c.gc)
    assert [v.v for v in c.layout(reg, [EL.Val(v) for v in x], EL.Val)] == outs
    assert [reg.advice.get(col.index) or [0] * 512 for col in c.gc.cs.advice] == cols


def test_the_recorders_keep_their_refusals():
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    c = _circuit(9, 4, "unsorted")
    reg = WP.LookupRecordingRegion(c.gc)
    with pytest.raises(WP.PlanError, match="a sort over values that are not assigned cells"):
        reg.sort_ascending([EL.Val(WP._Input(i)) for i in range(4)])
    rows = [(EL.Val(i), EL.Val(7 * i), EL.Val(i + 3)) for i in range(4)]
    with pytest.raises(WP.PlanError, match="shuffle.*data-dependent order"):
        reg.shuffle(rows, [EL.Val(WP._Input(0)), 1, 2, 3])
    mlp_reg = WP.RecordingRegion(EL.MlpCircuit(8, 2, [], [], 128, 2, n_inputs=3, relu_first=True).gc)
    for op, args in (("sort_ascending", ([],)), ("topk", ([], 1))):
        with pytest.raises(WP.PlanError, match=op):
            getattr(mlp_reg, op)(*args)
    with pytest.raises(AssertionError, match="sort key beyond 62 bits"):
        EL.BaseRegion(c.gc)._sorted([EL.Val(1), EL.Val(1 << 62)], "unsorted")
    with pytest.raises(AssertionError, match="sort key beyond 62 bits"):
        EL.BaseRegion(c.gc)._sorted([EL.Val(-(1 << 62)), EL.Val(0)], "largest_index_first")
    assert EL.BaseRegion(c.gc)._sorted([EL.Val((1 << 62) - 1), EL.Val(-(1 << 62) + 1), EL.Val((1 << 62) - 1)], "largest_index_first")[1] == [1, 2, 0]
