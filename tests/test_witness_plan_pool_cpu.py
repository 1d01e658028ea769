"""The ARGEXT record kind on the host: the interpreter (witness_plan.run_plan_host) against the closed form of tests/witness_synth_pool.py,
both validators on every plan and on the plans they must refuse, with the same words, the upload refusing those before a device is asked
for; PoolClassifierCircuit -- max and sum pooling -- recorded to the cells of the host layout; all rows of an `argmax_axes` in one ARGEXT
record; kinds 16, 23 and 26 refused as unknown; and the MLP recorder refusing the new ops by name."""
import ctypes as C

import numpy as np
import pytest

import witness_synth as S
import witness_synth_pool as T


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
        assert len(case.expect) == plan.n_cells and plan.records[:, 0].tolist() == [WP.INPUT, WP.ARGEXT] and not case.refused
        cols, outs = WP.run_plan_host(plan, case.x)
        _assert_columns(plan, cols, case.columns())
        assert outs == case.outputs()


def test_the_cases_plant_what_they_claim():
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    assert (WP.ARGEXT, WP.ARGEXT_CHUNK, WP.VERSION, WP.SORT_TILE) == (27, 4096, 1, 2048) and WP.ARGEXT_ERROR == EL.ARGEXT_ERROR
    assert [WP.kind_name(kd) for kd in (WP.ISQRT, 26, WP.ARGEXT, 28, 23, 16)] == ["sqrt", "?", "argext", "?", "?", "?"]
    assert T.LENGTHS == [1, 2, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193] and T.MANY == [(300, 5), (7, 64), (9, 100), (130, 1)]
    assert T.closed_form([2, 15, 2], 0) == 1 and T.closed_form([1, 1, 0], 0) == 0 and T.closed_form([3, -1, 5, -1], 1) == 1
    for mode in (0, 1):
        case = T.CASES["argext-n8193-mode%d" % mode](1)
        n = 8193
        vals = [S.signed(v % S.R) for v in case.x]
        seg = lambda name: vals[T.CONTENTS.index(name) * n:(T.CONTENTS.index(name) + 1) * n]
        want = [T.closed_form(seg(name), mode) for name in T.CONTENTS]
        assert want[T.CONTENTS.index("equal")] == 0 == case.outputs()[0] and case.outputs()[1] == want[-1]
        assert want[T.CONTENTS.index("ascending")] == (0 if mode else n - 1) and want[T.CONTENTS.index("descending")] == (n - 1 if mode else 0)
        assert want[T.CONTENTS.index("last")] == n - 1 and want[T.CONTENTS.index("tie63")] == 63 and want[T.CONTENTS.index("tie4095")] == 4095
        assert seg("tie63")[63] == seg("tie63")[64] and seg("tie4095")[4095] == seg("tie4095")[4096]
        assert {S.FIT - 1, -(S.FIT - 1)} <= set(seg("edges")) and max(seg("negative")) < 0 and set(seg("random")) == set(range(-3, 4))
        assert want[T.CONTENTS.index("edges")] in range(8)
    small = T.small_plan()
    assert small.columns()[1][:3] == [1, 2, 0], "argmin of [5, -2, 5, -2] is 1, of [3, 3, -7, 9] is 2"


@pytest.mark.parametrize("n", [100, T.CHUNK + 1])
def test_a_source_beyond_62_bits_is_named_with_the_smallest_element(parser, n):
    from ezkl_amd import witness_plan as WP
    good, bad = T.failing_case(n, False, seed=3), T.failing_case(n, True, seed=4)
    assert _check(parser, bad.plan.validate()) == 0 and bad.plan == good.plan
    cols, outs = WP.run_plan_host(good.plan, good.x)
    _assert_columns(good.plan, cols, good.columns())
    assert outs == good.outputs() and not good.refused
    assert bad.refused == [(1, n + e) for e in T.BAD_AT] and len(bad.unwritten) == 1 and bad.expect[bad.unwritten[0]] == 0
    with pytest.raises(AssertionError, match=r"%s \(argext record 1, element %d\)" % (WP.ARGEXT_ERROR, n + T.BAD_AT[0])):
        WP.run_plan_host(bad.plan, bad.x)


def test_both_validators_refuse_each_bad_shape_with_the_same_words(parser):
    from ezkl_amd import lib, witness_plan as WP
    H = lib.load()
    good = T.small_plan()
    assert _check(parser, good.plan.validate()) == 0
    cols, outs = WP.run_plan_host(good.plan, good.x)
    assert cols == good.columns() and outs == good.outputs() == [1, 2]
    seen = set()
    for words, rec, plan in T.bad_plans():
        assert WP.kind_name(plan.records[rec, 0]) == "argext"
        with pytest.raises(WP.PlanError) as e:
            WP.validate(plan)
        assert str(e.value) == "witness plan: record %d (argext): %s" % (rec, words)
        with pytest.raises(WP.PlanError, match=words):
            WP.run_plan_host(plan, good.x)
        assert _check(parser, plan) == -3, words
        assert parser.ezkl_prover_last_error().decode().endswith(str(e.value)), (words, parser.ezkl_prover_last_error())
        blob, h = plan.to_bytes(), C.c_void_p()
        assert H.ezkl_hip_witness_plan_upload(blob, C.c_size_t(len(blob)), C.byref(h)) == -3 and not h.value      # before a device is asked for
        assert H.ezkl_hip_witness_last_error().decode() == str(e.value)
        seen.add(words)
    assert seen == {"bad arg-extremum shape", "a cell is read before an earlier record has written it", "cell index out of range", "a cell is written twice"}


def test_kinds_16_23_and_26_and_the_new_end_are_refused_as_unknown(parser):
    from ezkl_amd import witness_plan as WP
    plan = T.small_plan().plan
    for kind in (16, 23, 26, 28, 0xFFFFFFFF):
        q = T._tampered(plan)
        q.records[1, 0] = kind
        with pytest.raises(WP.PlanError, match=r"record 1: unknown kind %d" % kind):
            WP.validate(q)
        assert _check(parser, q) == -3 and parser.ezkl_prover_last_error().decode().endswith("witness plan: record 1 (?): unknown kind")


# ---- recording ----------------------------------------------------------------------------------------------------------------------------
def _circuit(pool):
    from ezkl_amd import ezkl_layout as EL
    return EL.PoolClassifierCircuit(10, 2, 12000, pool=pool)


def _inputs(c, seed):
    return np.random.default_rng(seed).integers(0, 16, c.n_inputs).tolist()


@pytest.mark.parametrize("pool", ["max", "sum"])
def test_the_pool_classifier_records_to_the_cells_of_the_host_engine(parser, pool):
    from ezkl_amd import witness_plan as WP
    c = _circuit(pool)
    plan = WP.record_plan(c).validate()
    assert _check(parser, plan) == 0, parser.ezkl_prover_last_error().decode()
    assert WP.WitnessPlan.from_bytes(plan.to_bytes()) == plan and WP.peek(plan.to_bytes())["k"] == 10
    kinds = plan.records[:, 0].tolist()
    claims = [r for r in plan.records.tolist() if r[0] == WP.ARGEXT]
    assert len(claims) == 1 and claims[0][1:4] == [1, c.classes, 0], "one segment over the logits, argmax"
    assert WP.SORT in kinds and WP.ARGSORT in kinds and WP.GATHER in kinds and (WP.DIVC in kinds) == (pool == "sum")
    sorts = [r for r in plan.records.tolist() if r[0] == WP.SORT]
    assert sorted(r[2] for r in sorts) == ([4, 4] if pool == "max" else [4]), "the windows of the max pool share one SORT record"
    for seed in (1, 2, 3):
        x = _inputs(c, seed)
        adv, inst = _circuit(pool).witness(x)
        cols, outs = WP.run_plan_host(plan, x)
        for i, (got, want) in enumerate(zip(cols, adv)):
            assert got == want, "advice column %d differs on rows %s" % (i, [r for r in range(1 << 10) if got[r] != want[r]][:8])
        assert outs == inst[0] == [v % S.R for v in c.model(x)] and len(cols) == len(adv)


def test_all_rows_of_an_argmax_axes_share_one_record():
    from ezkl_amd import witness_plan as WP
    from test_pool_layout_cpu import arg_circuit
    rows = [[2, 15, 2, 15, 0], [1, 1, 0, 1, 1], [-4, -4, -4, -4, -4], [0, 1, 2, 3, 4]]
    x = [v for row in rows for v in row]
    for mode, want in (("max", [1, 0, 0, 4]), ("min", [4, 2, 0, 0])):
        plan = WP.record_plan(arg_circuit(4, 5, mode)).validate()
        claims = [r for r in plan.records.tolist() if r[0] == WP.ARGEXT]
        assert len(claims) == 1 and claims[0][1:4] == [4, 5, int(mode == "min")], "four segments of five: one launch"
        c = arg_circuit(4, 5, mode)
        reg = c.synthesize(x)
        cols, outs = WP.run_plan_host(plan, x)
        assert outs == c.outputs == want
        assert cols == [list(reg.advice.get(col.index) or [0] * (1 << c.k)) for col in c.gc.cs.advice]


@pytest.mark.parametrize("kind,geometry", [("max", (2, 4, 5, ((0, 0), (0, 0)), (2, 1), (2, 3))), ("sum", (2, 4, 5, ((1, 1), (1, 0)), (2, 2), (2, 2)))])
def test_the_pooling_ops_record_to_the_cells_of_the_host_engine(kind, geometry):
    """`max_pool` without padding (one SORT and one ARGSORT record for all its windows) and a padded, normalized `sumpool`"""
    from ezkl_amd import witness_plan as WP
    from test_pool_layout_cpu import pool_circuit
    make = lambda: pool_circuit(kind, *geometry, normalized=True)[0]
    plan = WP.record_plan(make()).validate()
    kinds = plan.records[:, 0].tolist()
    assert WP.ARGEXT not in kinds and (kinds.count(WP.SORT), kinds.count(WP.ARGSORT), kinds.count(WP.DIVC)) == ((1, 1, 0) if kind == "max" else (0, 0, 1))
    c = make()
    x = np.random.default_rng(5).integers(-40, 41, c.n_inputs).tolist()
    reg = c.synthesize(x)
    cols, outs = WP.run_plan_host(plan, x)
    assert outs == c.outputs and cols == [list(reg.advice.get(col.index) or [0] * (1 << c.k)) for col in c.gc.cs.advice]


def test_the_recorders_keep_their_refusals():
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    from test_pool_layout_cpu import arg_circuit, pool_circuit
    padded, _ = pool_circuit("max", 1, 3, 3, ((1, 0), (0, 0)), (1, 1), (2, 2))
    with pytest.raises(WP.PlanError, match="a sort over values that are not assigned cells"):
        WP.record_plan(padded)                                        # a padded window holds constants: laid out on the host only
    mlp_reg = WP.RecordingRegion(EL.MlpCircuit(8, 2, [], [], 128, 2, n_inputs=3, relu_first=True).gc)
    for op, args in (("argmax", ([],)), ("argmin", ([],)), ("select", ([], None)), ("max_pool", ([], 1, 1, 1, ((0, 0), (0, 0)), (1, 1), (1, 1))),
                     ("sumpool", ([], 1, 1, 1, ((0, 0), (0, 0)), (1, 1), (1, 1), False))):
        with pytest.raises(WP.PlanError, match="witness plans do not cover `%s`" % op):
            getattr(mlp_reg, op)(*args)
    reg = WP.LookupRecordingRegion(arg_circuit(1, 3, "max").gc)
    reg.decomp = (16, 2)
    with pytest.raises(WP.PlanError, match="an arg-extremum over values that are not assigned cells"):
        reg.argmax([EL.Val(WP._Input(i)) for i in range(3)])
