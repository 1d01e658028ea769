"""The record kinds of the surrogate's ops -- running sum and product, gather, clamp -- on the host: the interpreter
(witness_plan.run_plan_host) against the closed forms of tests/witness_synth_ops.py, both validators on every plan and on the plans they
must refuse, with the same words, the upload refusing those before a device is asked for; and the blobs of the circuit families that
were recorded before: their bytes have not moved."""
import ctypes as C
import hashlib

import pytest

import witness_synth as S
import witness_synth_ops as O

# the name a message gives every kind number below KINDS_TOP: "?" where the number is unassigned
KIND_NAMES = ["copy", "const", "input", "param", "add", "sub", "mult", "decompose", "range_check", "equals_zero", "dot", "nonlinearity", "nonlinearity_index", "matmul", "rlc", "div", "?",
              "sum", "prod", "gather", "clamp", "sort", "argsort", "?", "recip", "sqrt", "?", "argext", "?", "scatter", "complement", "one_hot"]


def _check(L, plan):
    blob = plan.to_bytes()
    return L.ezkl_prover_witness_plan_check(blob, C.c_size_t(len(blob)))


@pytest.fixture(scope="module")
def parser():
    from ezkl_amd import native
    return native.load()


@pytest.mark.parametrize("name", list(O.CASES))
def test_the_host_interpreter_equals_the_closed_form(parser, name):
    from ezkl_amd import witness_plan as WP
    for seed in (1, 2):
        case = O.CASES[name](seed)
        plan = case.plan.validate()
        assert _check(parser, plan) == 0, parser.ezkl_prover_last_error().decode()
        assert WP.WitnessPlan.from_bytes(plan.to_bytes()) == plan == O.CASES[name](seed).plan, "seeded: the same bytes again"
        assert len(case.expect) == plan.n_cells
        if case.refused:
            ri, el = case.refused[0]
            with pytest.raises(AssertionError, match=r"gather index outside the table \(gather record %d, element %d\)" % (ri, el)):
                WP.run_plan_host(plan, case.x)
            continue
        cols, outs = WP.run_plan_host(plan, case.x)
        want = case.columns()
        for c in range(plan.n_advice):
            assert cols[c] == want[c], "column %d differs on rows %s" % (c, [r for r in range(1 << plan.k) if cols[c][r] != want[c][r]][:8])
        assert outs == case.outputs()


def test_the_cases_plant_what_they_claim():
    """the value lists reach the edges the case names promise"""
    from ezkl_amd import witness_plan as WP
    R, H = S.R, S.HALF
    assert WP.KIND_NAMES == KIND_NAMES and (WP.SUMACC, WP.PRODACC, WP.GATHER, WP.CLAMP) == (17, 18, 19, 20) and WP.VERSION == 1
    assert 16 in WP.UNASSIGNED_KINDS and WP.DIVC == 15, "the kind after DIVC names nothing: tests/test_rebase_cpu.py holds both validators to that"
    assert {1, R - 1, H - 1, H + 1, (1 << 255) % R} <= set(O.SPECIAL) and (R - 1, R - 1) in zip(O.SPECIAL, O.SPECIAL[1:])
    ragged = O.CASES["prod-ragged-1-5-16-17-33"](1).plan
    assert ragged.records[1].tolist()[:4] == [WP.PRODACC, 5, 2, 33] and ragged.n_cells == len([v for v in S.field_operands(1) if v]) + 72
    assert int((ragged.pool[ragged.records[1, 4]:][:5 * 33] == S.NONE).sum()) == 5 * 33 - 72, "steps a shorter scan does not have"
    empty = O.CASES["sum-operandless-steps100"](1).plan
    a = empty.pool[empty.records[1, 5]:][:300].reshape(100, 3)
    assert [s for s in range(100) if (a[s] == S.NONE).all()] == [0, 6, 7, 13, 14, 99], "chunk = 7: the first step, both sides of two chunk edges, the last"
    bad = O.CASES["gather-outside-table300-lanes257"](1)
    wrong = O.gather_bad_indices(300)
    assert len(bad.refused) == len(wrong) == 16 and [S.signed(v) for v in wrong[:4]] == [-1, 300, 1 << 62, -(1 << 62)]
    assert all(any(v >> (32 * i) for v in wrong) for i in range(2, 8))
    idx = [S.signed(v) for v in O.CASES["gather-lanes65-table300"](1).plan.consts[300:]]
    assert 0 in idx and 299 in idx and all(0 <= v < 300 for v in idx)
    fan = [S.signed(v) for v in O.CASES["gather-fanin-table300"](1).plan.consts[300:]]
    assert max(fan.count(v) for v in (0, 1, 2)) > 60
    clamp = O.CASES["clamp-bounds-and-edges"](1)
    lo, hi = O.CLAMP_BOUNDS[0]
    assert {lo - 1, lo, 0, hi, hi + 1, -1, 1 << 62, -(1 << 62), H - 1, -(H + 1), -H} <= {S.signed(v) for v in clamp.plan.consts} and not clamp.refused
    assert {S.signed(v) for v in clamp.expect.values()} >= {lo, hi, 0, -1, -(1 << 31), (1 << 31) - 1}


@pytest.mark.parametrize("bad", [False, True])
def test_gather_failures_are_named_with_the_smallest_record_and_element(parser, bad):
    from ezkl_amd import witness_plan as WP
    case = O.gather_accounting_case(bad)
    assert _check(parser, case.plan.validate()) == 0 and case.plan == O.gather_accounting_case(not bad).plan
    if not bad:
        cols, outs = WP.run_plan_host(case.plan, case.x)
        assert cols == case.columns() and outs == case.outputs() and not case.refused
        return
    assert case.refused == [(2, 64), (2, 255), (3, 5), (3, 64), (3, 255), (3, 500)]
    with pytest.raises(AssertionError, match=r"gather index outside the table \(gather record 2, element 64\)"):
        WP.run_plan_host(case.plan, case.x)


def test_both_validators_refuse_each_bad_shape_with_the_same_words(parser):
    from ezkl_amd import lib, witness_plan as WP
    H = lib.load()
    good = O.small_plan()
    assert _check(parser, good.plan.validate()) == 0
    cols, outs = WP.run_plan_host(good.plan, good.x)
    assert cols == good.columns() and outs == good.outputs() == [5]
    seen = set()
    for words, rec, plan in O.bad_plans():
        name = WP.KIND_NAMES[plan.records[rec, 0]]
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
    assert {"bad scan shape", "gather table runs past the pool", "empty gather table", "bad clamp bounds"} <= seen


def test_the_blobs_of_the_earlier_families_keep_their_bytes():
    """the kinds are appended and the version word stays 1: an MLP, a conv and a standalone einsum circuit record to the bytes the
    existing tests pin (their digests, taken on the commits those files name), and to no record of a new kind"""
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


# ---- recording: sum / prod, the surrogate ---------------------------------------------------------------------------------------------------
CHAL = [12345678901234567890123 % S.R, 98765432109876543210 % S.R]     # the two challenges of tests/test_transformer_surrogate.py


# k = 6: 57 usable rows to a column.  (w, length): a sum that ends inside a row (7 of w = 2, 23 of w = 3), on a row (40 of w = 2, 9 of
# w = 1, 24 of w = 3), and past a column boundary -- the duplicated row -- (70 of w = 1, 130 of w = 2, 100 of w = 3)
SUM_PROD_SHAPES = [(1, 9), (2, 7), (2, 40), (3, 23), (3, 24), (1, 70), (2, 130), (3, 100)]


@pytest.mark.parametrize("w,length", SUM_PROD_SHAPES)
def test_sum_and_prod_record_to_the_cells_of_the_host_engine(parser, w, length):
    import numpy as np
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    x = np.random.default_rng(w * 100 + length).integers(-9, 10, length).tolist()
    c = EL.SumProdLayoutCircuit(6, w, 7 * length + 32, length)
    plan = WP.record_plan(c).validate()
    assert _check(parser, plan) == 0, parser.ezkl_prover_last_error().decode()
    kinds = plan.records[:, 0].tolist()
    assert kinds.count(WP.SUMACC) == 2 and kinds.count(WP.PRODACC) == 1
    adv, inst = c.witness(x)
    cols, outs = WP.run_plan_host(plan, x)
    for i, (got, want) in enumerate(zip(cols, adv)):
        assert got == want, "advice column %d differs on rows %s" % (i, [r for r in range(64) if got[r] != want[r]][:8])
    assert outs == inst[0] and len(cols) == len(adv)
    parent = EL.SumProdCircuit(6, w, 7 * length + 32)
    assert parent.witness(x) == (adv, inst), "the subclass lays out its parent's cells"
    reg, preg = c.synthesize(x), parent.synthesize(x)
    assert reg.copies == preg.copies and [None if a is None else a.tolist() for a in reg.activations] == [None if a is None else a.tolist() for a in preg.activations]


def test_the_sum_and_prod_shapes_reach_the_duplicated_row():
    """a step without operands is the running value duplicated at the top of a new column: the long shapes have one, the short ones none"""
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    def duplicated(w, length):
        plan = WP.record_plan(EL.SumProdLayoutCircuit(6, w, 7 * length + 32, length))
        return any((plan.pool[r[5]:r[5] + r[1] * r[2] * r[3]].reshape(r[3], r[2]) == S.NONE).all(1).any() for r in plan.records.tolist() if r[0] in (WP.SUMACC, WP.PRODACC))
    assert [duplicated(w, n) for w, n in SUM_PROD_SHAPES] == [False, False, True, False, False, True, True, True]


def test_the_recorders_keep_their_refusals():
    import numpy as np
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    with pytest.raises(WP.PlanError, match="SumProdCircuit"):
        WP.record_plan(EL.SumProdCircuit(8, 1, 400))
    mlp_reg = WP.RecordingRegion(EL.MlpCircuit(8, 2, [], [], 128, 2, n_inputs=3, relu_first=True).gc)
    for op, args in (("sum", ([],)), ("prod", ([],)), ("dynamic_lookup", ([], [])), ("shuffle", ([], []))):
        with pytest.raises(WP.PlanError, match=op):
            getattr(mlp_reg, op)(*args)
    c = _surrogate(9)
    reg = WP.LookupRecordingRegion(c.gc)
    rows = [(EL.Val(i), EL.Val(7 * i), EL.Val(i + 3)) for i in range(4)]
    with pytest.raises(WP.PlanError, match="shuffle.*data-dependent order"):
        reg.shuffle(rows, [EL.Val(WP._Input(0)), 1, 2, 3])
    with pytest.raises(WP.PlanError, match="keys are not its positions"):
        reg.row_at([(EL.Val(i + 1), EL.Val(0), EL.Val(0)) for i in range(4)], EL.Val(WP._Input(0)))
    reg.shuffle(rows, np.array([3, 1, 0, 2]))                       # an integer order records: constants on both sides
    assert {r["kind"] for r in reg.out.recs} == {WP.CONST}


def _surrogate(k):
    from ezkl_amd import ezkl_layout as EL
    return EL.TransformerSurrogateCircuit(k, blocks=2, d=4, einsum_len=3, decomp_base=16, lookup_max=(1 << k) // 16)


def other_inputs(c, seed=7):
    """a second input vector of the surrogate: other x, tokens, A and B"""
    import numpy as np
    rng = np.random.default_rng(seed)
    x = rng.integers(-9, 10, c.d).tolist() + rng.integers(0, 8, 2 * c.d).tolist() + rng.integers(-8, 8, 2 * c.L * c.L).tolist()
    assert x != c.default_inputs() and len(x) == c.n_inputs == 3 * c.d + 2 * c.L * c.L
    return x


def tiled_plan_columns(c, plan, built, x):
    """the plan through the host interpreter, phase 0 then phase 1 under CHAL, tiled here with numpy: the circuit's columns as ints"""
    import numpy as np
    from ezkl_amd import witness_plan as WP
    U, T, n = built["info"]["unit_rows"], built["info"]["tiles"], 1 << c.k
    first, _ = WP.run_plan_host(plan, x, phase=0)
    cols, outs = WP.run_plan_host(plan, x, challenges=CHAL)
    phases = WP.column_phases(plan)
    assert all(cols[i] == first[i] for i in range(plan.n_advice) if phases[i] == 0) and all(not any(first[i]) for i in range(plan.n_advice) if phases[i] == 1)
    src = {cb: c0 for c0, cbs in c._colmap.items() for cb in cbs}
    out = []
    for i in range(plan.n_advice):
        unit = np.array(cols[src.get(i, i)], dtype=object)
        assert not unit[U:].any() and (i not in src or src[i] == i or not any(cols[i])), "the plan writes the unit rows of the block-0 and shared columns only"
        out.append(np.concatenate([np.tile(unit[:U], T), np.zeros(n - T * U, dtype=object)]).tolist())
    return out, outs


@pytest.mark.parametrize("k", [9, 10])
def test_the_surrogate_records_to_the_columns_of_the_host_layout(parser, k):
    from ezkl_amd import witness_plan as WP
    from oracle import mock_prover as MP
    c = _surrogate(k)
    plan = WP.record_plan(c).validate()
    assert _check(parser, plan) == 0, parser.ezkl_prover_last_error().decode()
    assert (plan.n_phases, plan.n_challenges, plan.n_inputs) == (2, 2, 3 * 4 + 2 * 9) and plan.n_records == WP.record_plan(_surrogate(19 - k)).n_records
    kinds = plan.records[:, 0].tolist()
    assert {WP.SUMACC, WP.GATHER, WP.CLAMP, WP.MATMUL, WP.RLC, WP.TABLE, WP.PARAM} <= set(kinds) and kinds.count(WP.MATMUL) == 1
    assert all(ph == (1 if kind == WP.RLC else ph) for kind, ph in zip(kinds, plan.records[:, 7].tolist())) and sorted(plan.records[:, 7].tolist()) == plan.records[:, 7].tolist()
    assert len(plan.params) == 2 * 16 + 4 + 3 * 8 + 3 * 8, "Wq, W2, b2, the embedding rows, perm_rows"
    for x in (None, other_inputs(c)):
        cb = _surrogate(k)                                            # (a build compresses its circuit's selectors in place: one circuit each)
        built = cb.build(as_ints=True, inputs=x)
        got, outs = tiled_plan_columns(cb, plan, built, c.default_inputs() if x is None else x)
        cs = built["cs"]
        want0, want1 = built["advice"](0, []), built["advice"](1, CHAL)
        for i in range(cs.n_advice):
            want = list((want0 if cs.advice_phase[i] == 0 else want1)[i])
            assert got[i] == want, "advice column %d differs on rows %s" % (i, [r for r in range(1 << k) if got[i][r] != want[r]][:8])
        assert outs == built["instances"][0]
        if x is not None:
            assert MP.check(cs, got, [list(f) for f in built["fixed"]], built["instances"], list(built["copies"]), CHAL) == []
            assert built["instances"] != _surrogate(k).build(as_ints=True)["instances"]


@pytest.mark.parametrize("token", [8, -1])
def test_a_token_outside_the_table_fails_the_layout_and_the_interpreter_by_name(token):
    from ezkl_amd import witness_plan as WP
    c = _surrogate(9)
    x = c.default_inputs()
    x[c.d + 3] = token
    with pytest.raises(AssertionError, match="gather index outside the table"):
        c.build(as_ints=True, inputs=x)
    plan = WP.record_plan(c)
    gathers = [ri for ri, r in enumerate(plan.records.tolist()) if r[0] == WP.GATHER]
    assert len(gathers) == 2 and plan.records[gathers[0], 3] == 8, "one record per embedding coordinate, over the 8 rows of the table"
    with pytest.raises(AssertionError, match=r"gather index outside the table \(gather record %d, element 3\)" % gathers[0]):
        WP.run_plan_host(plan, x, challenges=CHAL)
