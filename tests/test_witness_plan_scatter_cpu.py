"""The SCATTER, COMPLEMENT and ONEHOT record kinds on the host: the interpreter (witness_plan.run_plan_host) against the closed form of
tests/witness_synth_scatter.py, both validators on every plan and on the plans they must refuse, with the same words, the upload refusing
those before a device is asked for; ScatterGatherCircuit and one-op circuits recorded to the cells of the host layout -- one SCATTER, one
COMPLEMENT, the ONEHOT elements in one record, the picks of a `select_elements` in one GATHER record --; kinds 16, 23, 26, 28 and the new end
refused as unknown; and the recorders' refusals by name."""
import ctypes as C
import re

import numpy as np
import pytest

import witness_synth as S
import witness_synth_scatter as T
from test_witness_plan_pool_cpu import _assert_columns, _check


@pytest.fixture(scope="module")
def parser():
    from ezkl_amd import native
    return native.load()


@pytest.mark.parametrize("name", list(T.CASES))
def test_the_host_interpreter_equals_the_closed_form(parser, name):
    from ezkl_amd import witness_plan as WP
    for seed in (1, 2):
        case = T.CASES[name](seed)
        plan = case.plan.validate()
        assert _check(parser, plan) == 0, parser.ezkl_prover_last_error().decode()
        assert WP.WitnessPlan.from_bytes(plan.to_bytes()) == plan == T.CASES[name](seed).plan, "seeded: the same bytes again"
        assert len(case.expect) == plan.n_cells and set(plan.records[:, 0].tolist()) <= {WP.INPUT, WP.SCATTER, WP.COMPLEMENT, WP.ONEHOT}
        if case.refused:
            ri, el = case.refused[0]
            with pytest.raises(AssertionError, match=re.escape("%s (one_hot record %d, element %d)" % (WP.ONEHOT_ERROR, ri, el))):
                WP.run_plan_host(plan, case.x)
            continue
        cols, outs = WP.run_plan_host(plan, case.x)
        _assert_columns(plan, cols, case.columns())
        assert outs == case.outputs()


def test_a_complement_of_more_tiles_than_lanes(parser):
    from ezkl_amd import witness_plan as WP
    case = T.offsets_case(1)
    plan = case.plan.validate()
    assert _check(parser, plan) == 0 and plan.records[1].tolist()[:4] == [WP.COMPLEMENT, 256 * T.TILE + 1 - 800, 256 * T.TILE + 1, 800]
    cols, outs = WP.run_plan_host(plan, case.x)
    assert cols == case.columns() and outs == case.outputs() and outs[1] == 256 * T.TILE - 300


def test_the_cases_plant_what_they_claim():
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    assert (WP.SCATTER, WP.COMPLEMENT, WP.ONEHOT, WP.KINDS_TOP, WP.SCATTER_TILE, WP.VERSION) == (29, 30, 31, 32, T.TILE, 1)
    assert (WP.SCATTER_ERROR, WP.ONEHOT_ERROR) == (EL.SCATTER_ERROR, EL.ONEHOT_ERROR) == ("scatter index outside the tensor", "one-hot index outside the classes")
    assert [WP.kind_name(kd) for kd in (WP.SCATTER, WP.COMPLEMENT, WP.ONEHOT, 28, 32)] == ["scatter", "complement", "one_hot", "?", "?"]
    assert T.SIZES == [1, 2, 63, 64, 65, 255, 256, 257, T.TILE - 1, T.TILE, T.TILE + 1, 2 * T.TILE + 1]
    small = T.small_plan()
    cols = small.columns()
    assert cols[1][:6] == [1, 20, 3, 4, 10, 6], "index [2, 0] along dim 0 of a 3 x 2 tensor: (2, 0) <- 10, (0, 1) <- 20"
    assert cols[2][:7] == [1, 3, 4, 5, 1, 0, 0], "{0 .. 5} without {2, 0}, then the one-hot vector of 0 over three classes"
    n = 2 * T.TILE + 1
    case = T.CASES["scatter-n%d" % n](1)
    recs = [r for r in case.plan.records.tolist() if r[0] == WP.SCATTER]
    assert [r[1] for r in recs] == [n] * len(T.SCATTER_CONTENTS) and recs[2][2] == n + 3, "onto-one: more elements than cells"
    assert recs[6][3] == 3 and recs[7][3] == 1, "the 2-D cases: multiplier 3 along dim 0, 1 along dim 1"
    pool = case.plan.pool.tolist()
    assert any(pool[recs[7][6] + 1 + 2 * recs[7][2] + j] for j in range(recs[7][2])), "non-zero offsets"
    case = T.CASES["complement-n%d" % n](1)
    recs = [r for r in case.plan.records.tolist() if r[0] == WP.COMPLEMENT]
    assert [(r[1], r[3]) for r in recs] == [(n, 0), (0, n), (n // 2, n - n // 2), (n - n // 3, n // 3), (n - n // 3, n // 3), (n - 8, 8)]
    got = case.columns()
    cell = lambda c: got[c >> case.plan.k][c & ((1 << case.plan.k) - 1)]
    outside = sorted(cell(c) for c in case.plan.pool[recs[5][4]:recs[5][4] + recs[5][1]].tolist())
    assert outside == [v for v in range(1, n) if v != n // 2][:n - 8], "duplicates and outsiders remove nothing: the last of the set are cut off"
    bad = T.CASES["onehot-outside"](1)
    assert len(bad.refused) == (1 + 2 + 65) * 4 and len(bad.unwritten) == len(bad.refused)


@pytest.mark.parametrize("n", [100, T.TILE + 1])
def test_a_failing_scatter_leaves_all_its_cells_and_is_named_with_the_smallest_element(parser, n):
    from ezkl_amd import witness_plan as WP
    good, bad = T.failing_case(n, False, seed=3), T.failing_case(n, True, seed=4)
    assert _check(parser, bad.plan.validate()) == 0 and bad.plan == good.plan
    cols, outs = WP.run_plan_host(good.plan, good.x)
    _assert_columns(good.plan, cols, good.columns())
    assert outs == good.outputs() and not good.refused
    ri = 6                                                            # the middle scatter: the base, then INPUT, INPUT, SCATTER per tensor
    assert [r[0] for r in bad.plan.records.tolist()] == [WP.INPUT] + [WP.INPUT, WP.INPUT, WP.SCATTER] * 3
    assert bad.refused == [(ri, e) for e in T.BAD_AT] and len(bad.unwritten) == n and all(bad.expect[c] == 0 for c in bad.unwritten)
    assert sum(1 for c, v in bad.expect.items() if v) > 2 * n, "the neighbours' cells are written"
    with pytest.raises(AssertionError, match=re.escape("%s (scatter record %d, element %d)" % (WP.SCATTER_ERROR, ri, T.BAD_AT[0]))):
        WP.run_plan_host(bad.plan, bad.x)


def test_both_validators_refuse_each_bad_shape_with_the_same_words(parser):
    from ezkl_amd import lib, witness_plan as WP
    H = lib.load()
    good = T.small_plan()
    assert _check(parser, good.plan.validate()) == 0
    cols, outs = WP.run_plan_host(good.plan, good.x)
    assert cols == good.columns() and outs == good.outputs()
    seen = set()
    for words, rec, plan in T.bad_plans():
        name = WP.kind_name(plan.records[rec, 0])
        assert name == {3: "scatter", 4: "complement", 5: "one_hot"}[rec]
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
    assert seen == {"bad scatter shape", "bad complement shape", "zero one-hot classes", "a cell is read before an earlier record has written it",
                    "cell index out of range", "a cell is written twice"}


def test_an_empty_complement_is_legal_and_every_other_empty_record_is_not(parser):
    from ezkl_amd import witness_plan as WP
    case = T.CASES["complement-n2"](1)
    empty = [ri for ri, r in enumerate(case.plan.records.tolist()) if r[0] == WP.COMPLEMENT and r[1] == 0]
    assert empty and _check(parser, case.plan.validate()) == 0
    q = T._tampered(case.plan)
    q.records[empty[0], 0] = WP.COPY
    with pytest.raises(WP.PlanError, match="record %d is empty" % empty[0]):
        WP.validate(q)
    assert _check(parser, q) == -3 and parser.ezkl_prover_last_error().decode().endswith("record %d (copy): empty" % empty[0])


def test_the_unassigned_kinds_and_the_new_end_are_refused_as_unknown(parser):
    from ezkl_amd import witness_plan as WP
    plan = T.small_plan().plan
    for kind in (16, 23, 26, 28, WP.KINDS_TOP, 0xFFFFFFFF):
        q = T._tampered(plan)
        q.records[3, 0] = kind
        assert WP.kind_name(kind) == "?"
        with pytest.raises(WP.PlanError, match=r"record 3: unknown kind %d" % kind):
            WP.validate(q)
        assert _check(parser, q) == -3 and parser.ezkl_prover_last_error().decode().endswith("witness plan: record 3 (?): unknown kind")


# ---- recording ----------------------------------------------------------------------------------------------------------------------------
def _circuit():
    from ezkl_amd import ezkl_layout as EL
    return EL.ScatterGatherCircuit(10, 2, 6000)


def inputs(c, seed):
    """a table, an index with distinct values in every column, a source and the picks"""
    rng = np.random.default_rng(seed)
    index = np.stack([rng.permutation(c.rows)[:c.m] for _ in range(c.cols)], 1).reshape(-1)
    return np.concatenate([rng.integers(-50, 51, c.rows * c.cols), index, rng.integers(-50, 51, c.m * c.cols), rng.integers(0, c.rows, c.picks)]).tolist()


def _host_columns(c, x):
    reg = c.synthesize(x)
    return [list(reg.advice.get(col.index) or [0] * (1 << c.k)) for col in c.gc.cs.advice]


def test_the_scatter_gather_circuit_records_to_the_cells_of_the_host_engine(parser):
    from ezkl_amd import witness_plan as WP
    c = _circuit()
    plan = WP.record_plan(c).validate()
    assert _check(parser, plan) == 0, parser.ezkl_prover_last_error().decode()
    assert WP.WitnessPlan.from_bytes(plan.to_bytes()) == plan and WP.peek(plan.to_bytes())["k"] == 10
    recs = plan.records.tolist()
    by_kind = lambda kind: [r for r in recs if r[0] == kind]
    n = c.rows * c.cols
    assert [r[1:4] for r in by_kind(WP.SCATTER)] == [[n, c.m * c.cols, c.cols]], "one SCATTER: n cells, m x cols elements, multiplier cols"
    assert [r[1:4] for r in by_kind(WP.COMPLEMENT)] == [[n - c.m * c.cols, n, c.m * c.cols]], "one COMPLEMENT"
    assert [r[1:3] for r in by_kind(WP.ONEHOT)] == [[2 * c.rows, c.rows]], "the claim on the output VarTensor and beside its range check: one record"
    gathers = sorted(r[1] for r in by_kind(WP.GATHER))
    assert gathers == sorted([c.m * c.cols, n - c.m * c.cols, c.picks * c.cols, 1]), "every `select_elements` is one GATHER record"
    for seed in (1, 2, 3):
        x = inputs(c, seed)
        adv, inst = _circuit().witness(x)
        cols, outs = WP.run_plan_host(plan, x)
        for i, (got, want) in enumerate(zip(cols, adv)):
            assert got == want, "advice column %d differs on rows %s" % (i, [r for r in range(1 << 10) if got[r] != want[r]][:8])
        assert outs == inst[0] == [v % S.R for v in c.model(x)] and len(cols) == len(adv)


def op_circuit(name):
    """one op of the family on a private vector"""
    from ezkl_amd import ezkl_layout as EL
    from test_pool_layout_cpu import OpCircuit
    if name == "scatter-2d-dim1":                                      # a 3 x 4 tensor, a 3 x 2 index along dim 1, its source
        op = lambda reg, v: reg.scatter_elements(v[:12], [3, 4], v[12:18], [3, 2], v[18:24], 1)
        return OpCircuit(24, 12, op, sorts=2, sort_rows=18, selects=3, select_rows=36, k=10, capacity=6000)
    if name == "gather_elements":                                      # the 2 x 2 example along dim 1
        op = lambda reg, v: reg.gather_elements(v[:4], [2, 2], v[4:8], [2, 2], 1)[0]
        return OpCircuit(8, 4, op, selects=1, select_rows=4)
    if name == "one_hot_axis":                                         # two indices over four classes, the classes as the LAST axis
        op = lambda reg, v: reg.one_hot_axis(v, [2], 4, 1)
        return OpCircuit(2, 8, op, selects=2, select_rows=8)
    op = lambda reg, v: reg.get_missing_set_elements(v, [EL.Val(j, const=True) for j in range(7)], name == "missing-ordered")
    return OpCircuit(3, 4, op, sorts=2, sort_rows=11, k=10, capacity=6000)


OP_INPUTS = {"scatter-2d-dim1": list(range(12)) + [3, 0, 1, 2, 0, 3] + [50, 51, 52, 53, 54, 55], "gather_elements": [1, 2, 3, 4, 0, 0, 1, 0], "one_hot_axis": [3, 0],
             "missing-ordered": [5, 0, 3], "missing-unordered": [6, 1, 2]}


@pytest.mark.parametrize("name", list(OP_INPUTS))
def test_one_op_circuits_record_to_the_cells_of_the_host_engine(name):
    from ezkl_amd import witness_plan as WP
    plan = WP.record_plan(op_circuit(name)).validate()
    kinds = plan.records[:, 0].tolist()
    want = {"scatter-2d-dim1": (1, 1, 0), "gather_elements": (0, 0, 0), "one_hot_axis": (0, 0, 1), "missing-ordered": (0, 1, 0), "missing-unordered": (0, 1, 0)}[name]
    assert (kinds.count(WP.SCATTER), kinds.count(WP.COMPLEMENT), kinds.count(WP.ONEHOT)) == want
    assert (kinds.count(WP.SORT), kinds.count(WP.ARGSORT)) == ((1, 1) if name in ("scatter-2d-dim1", "missing-ordered") else (0, 0))
    x = OP_INPUTS[name]
    c = op_circuit(name)
    cols, outs = WP.run_plan_host(plan, x)
    assert cols == _host_columns(c, x) and outs == c.outputs
    if name == "gather_elements":
        assert outs == [1, 1, 4, 3] and kinds.count(WP.GATHER) == 1 and [r[1] for r in plan.records.tolist() if r[0] == WP.GATHER] == [4]
    if name == "one_hot_axis":
        assert outs == [0, 0, 0, 1, 1, 0, 0, 0]
    if name.startswith("missing"):
        assert sorted(outs) == sorted(set(range(7)) - set(x)) and (name == "missing-unordered" or outs == sorted(outs))


def test_the_recorders_keep_their_refusals():
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    Val = EL.Val
    mlp_reg = WP.RecordingRegion(EL.MlpCircuit(8, 2, [], [], 128, 2, n_inputs=3, relu_first=True).gc)
    for op, args in (("select_elements", ([], [])), ("linearize_element_index", ([], [1], 0, True)), ("gather", ([], [1], [], 0)), ("gather_elements", ([], [1], [], [1], 0)),
                     ("one_hot", (None, 2)), ("one_hot_axis", ([], [0], 2, 0)), ("shuffles", ([], [])), ("get_missing_set_elements", ([], [], True)),
                     ("scatter_elements", ([], [1], [], [1], [], 0))):
        with pytest.raises(WP.PlanError, match="witness plans do not cover `%s`" % op):
            getattr(mlp_reg, op)(*args)
    fresh = lambda: WP.LookupRecordingRegion(op_circuit("missing-ordered").gc)
    cells = lambda reg, n: reg.assign(reg.inputs[0], [Val(WP._Input(i)) for i in range(n)])
    reg = fresh()
    with pytest.raises(WP.PlanError, match=re.escape("a missing-set over a full set that is not the positions 0 .. n - 1")):
        reg.get_missing_set_elements(cells(reg, 2), [Val(j, const=True) for j in (0, 2, 1)], False)
    reg = fresh()
    with pytest.raises(WP.PlanError, match=re.escape("a missing-set over a full set that is not the positions 0 .. n - 1")):
        reg.shuffles(cells(reg, 3), [Val(j + 1, const=True) for j in range(3)])
    reg = fresh()
    with pytest.raises(WP.PlanError, match="a missing-set over values that are not assigned cells"):
        reg.get_missing_set_elements([Val(WP._Input(0))], [Val(j, const=True) for j in range(3)], False)
    reg = fresh()
    with pytest.raises(WP.PlanError, match="a one-hot over an index that is not an assigned cell"):
        reg.one_hot(Val(WP._Input(0)), 3)
    for hole in (0, 2):                                               # a base or a source that is not an assigned cell: refused by name (an index is assigned by the op)
        reg = fresh()
        parts = [cells(reg, 3), None, None]
        reg.increment(3)
        parts[1] = cells(reg, 2)
        reg.increment(2)
        parts[2] = cells(reg, 2)
        reg.increment(2)
        parts[hole] = [Val(7, const=True)] * len(parts[hole])
        with pytest.raises(WP.PlanError, match="a scatter over values that are not assigned cells"):
            reg.scatter_elements(parts[0], [3], parts[1], [2], parts[2], 0)
