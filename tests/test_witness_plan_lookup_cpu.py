"""Witness plans with static lookups, without a GPU (ezkl_amd/witness_plan.py): the layout of a ConvMnistCircuit -- conv as dot + bias per
output, ReLU by decomposition, Div{denom} through a static lookup table, a linear layer -- recorded once from the circuit's own `layout`
and replayed by `run_plan_host` must reproduce `circuit.witness(img)` in every advice column and in the outputs.  The records follow
dependence levels (their number does not grow with the image), a lookup input outside its table is reported with its record and element,
hand-built plans cover the table ends and the negative side no conv circuit reaches (ReLU feeds the lookup), and both validators -- the
Python mirror and csrc/witness_plan.hpp through libezkl_prover.so -- refuse a bad table section with the same words.  MLP plans keep
the bytes they had before the format learnt tables."""
import hashlib

import numpy as np
import pytest

from test_witness_plan_cpu import CASES as MLP_CASES, _mlp

# name -> (records, sha256 of record_plan(circuit).to_bytes(), the first 16 hex digits of params_hash(circuit)).  The MLP rows are the cases
# of tests/test_witness_plan_cpu.py; mlp_k9_w2's digest was taken on commit 05df2094cb08ff47267e800d503f02d542bd0088, the last one whose
# plan format had no table section, every other figure on commit 50e40f7, the last one whose recorder restated the MLP's op sequence and
# packed its parameters itself (there mlp_k9_w2 still had the digest of 05df209)
MLP_PINS = {
    "golden_k6_5_blocks": (52, "ffe47266be64e9c78ee373572843f7e77f7a0d53d665e86e509cfa117c56b1e0", "8adc4d7fb3f4fcdf"),
    "mlp_k9_w2_3_blocks": (98, "b352394d5d9bb4650f74b8253d9c35401ec15b1721734fb292121a46b6cda58a", "32d93f091822c46c"),
    "mlp_k9_w1_5_blocks": (98, "621528fd4387d381fb30dcdf417c1545cb445b6cf808f4108d14e76d4e17f77f", "7770728dbcb89168"),
    "1l_relu_k8": (46, "fe1787de709d463145514ed530d7681334c07f98cb75def100d5ca8182f9aa35", "a1bd617a1d2e51fa"),
    "mlp_k9_w2_no_relu_last_2_blocks": (79, "c71aba0e0428a819d0e105d727e06c5a434d4cda75803ac90536d09e9d51e70a", "b6c1e1f0454241fa"),
    "1l_relu_k8_w1": (46, "3023bb14d07f5059e7165fd428676dbf2a022b666f65020ce7a48f873011d13c", "8a664557d6a8a4c9"),
    "mlp_k7_w1_dot_crosses_a_column_top": (75, "f3ec7c4de427912cb7fefe2afae30b68efd7e7bc43f1d70bffe04dd14c488642", "3c9e48c40b666896"),
    "mlp_k7_w2_dot_crosses_a_column_top": (75, "7b1f029195b409ab32b27d053de8d2c78892513118dc2d41640c5c8ff0edeabf", "a7b4be905d566f60"),
}
CONV_PINS = {
    "conv_k10_w1": (31, "ff0aa0f09047756db62b068c211d991aa70c43e82c45bf45cf658448453f86d7", "69e83bedafaccb66"),
    "conv_k10_w2": (31, "1c035ddcdf5d92165b1b65577210bd1cb75508ae3e36c07527597f192583547a", "3390acee145d45f8"),
    "conv_k6_w1_4_blocks_4_table_columns": (31, "c807c7eb5eec3cf379ec375ec27b17ba06ac9a5ed198cf01c7e0ef0a18dc8825", "977044005eb45851"),
    "conv_k6_w2_2_blocks_4_table_columns": (31, "987b271317c69abcd9454589b50fdb6f8120b38911b4a7813393cb982f6c966f", "871bb318bf19bebc"),
}


def _case_a(w):
    """tests/test_ezkl_circuit.py::_conv_small, with one or two inner columns: the linear coordinate ends at 607 / 643"""
    from ezkl_amd import ezkl_layout as EL
    c = EL.ConvMnistCircuit(logrows=10, image=8, kernel=3, out_channels=2, stride=2, classes=3, lookup_range=(-700, 700), denom=4,
                            decomp_base=32, decomp_legs=2, num_inner_cols=w)
    rng = np.random.default_rng(1)
    c.kernels = rng.integers(-3, 4, c.kernels.shape)
    return c, rng.integers(0, 4, (8, 8))


def _case_b(w, levels=(0, 1, 2, 3)):
    """the k = 6 circuit of test_conv2d_mnist_tiny_proof_oracle_backend with every kernel entry 3 and an image of four constant 3 x 3
    quadrants: the lookup inputs are 27 * level, over a Div{4} table of four columns (col_size 56) -- levels 0..3 give the table-column
    indices 1, 2, 2, 3; the VarTensors overflow into 4 blocks (w = 1) / 2 blocks (w = 2), so the dots cross column tops"""
    from ezkl_amd import ezkl_layout as EL
    c = EL.ConvMnistCircuit(logrows=6, image=6, kernel=3, out_channels=1, stride=3, classes=2, lookup_range=(-100, 100), denom=4,
                            decomp_base=16, decomp_legs=2, capacity=220, num_inner_cols=w)
    rng = np.random.default_rng(2)                                # (the kernels are constant here: fc_w / fc_b are the generator's first draws)
    c.fc_w, c.fc_b = rng.integers(-5, 6, c.fc_w.shape), rng.integers(-9, 10, c.fc_b.shape)
    c.kernels = np.full(c.kernels.shape, 3)
    img = np.kron(np.array(levels).reshape(2, 2), np.ones((3, 3), np.int64))
    return c, img


def _case_c():
    from ezkl_amd import ezkl_layout as EL
    return EL.ConvMnistCircuit(), np.random.default_rng(3).integers(0, 16, (28, 28))


CASES = {
    "conv_k10_w1": lambda: _case_a(1),
    "conv_k10_w2": lambda: _case_a(2),
    "conv_k6_w1_4_blocks_4_table_columns": lambda: _case_b(1),
    "conv_k6_w2_2_blocks_4_table_columns": lambda: _case_b(2),
    "conv_mnist_k17": _case_c,
}


def _signed(v):
    from ezkl_amd import ezkl_layout as EL
    return v if v < EL.R // 2 else v - EL.R


@pytest.mark.parametrize("name", list(CASES))
def test_host_interpreter_reproduces_the_conv_layout(name):
    from ezkl_amd import witness_plan as WP
    circuit, img = CASES[name]()
    adv, inst = circuit.witness(img)
    plan = WP.record_plan(circuit)
    cols, outs = WP.run_plan_host(plan, img.reshape(-1))
    assert len(cols) == len(adv) == plan.n_advice
    for c, (mine, ref) in enumerate(zip(cols, adv)):
        assert mine == ref, "advice column %d differs" % c
    assert [outs] == inst and [_signed(v) for v in outs] == circuit.model(img)
    assert plan.n_cells >= sum(1 for col in adv for v in col if v)
    kinds = plan.records[:, 0].tolist()
    assert kinds.count(WP.TABLE) == 1 and kinds.count(WP.TBLIDX) == 1 and len(plan.tables) == 1
    lo, n, col_size, off = plan.tables[0]
    table = circuit.gc.base.static_tables["div_%d" % circuit.denom]
    assert (lo, lo + n - 1, col_size, off) == (table.range[0], table.range[1], table.col_size, 0) and len(plan.table_values) == n
    # a second input reuses the plan
    img2 = (img + 1) % 4
    cols2, outs2 = WP.run_plan_host(plan, img2.reshape(-1))
    adv2, inst2 = circuit.witness(img2)
    assert cols2 == adv2 and [outs2] == inst2
    # deterministic, and the blob round-trips
    blob = plan.to_bytes()
    assert WP.record_plan(CASES[name]()[0]).to_bytes() == blob
    again = WP.WitnessPlan.from_bytes(blob)
    assert again.to_bytes() == blob and again == plan and again.tables == plan.tables
    assert plan.param_hash == WP.params_hash(circuit) and WP.peek(blob)["n_tables"] == 1 and WP.peek(blob)["n_table_values"] == n
    if name.startswith("conv_k6"):
        assert [_signed(v) for v in outs] == [-120, -71]
        assert circuit.gc.advices[0].num_blocks() == (4 if circuit.w == 1 else 2)
        assert len(table.table_inputs) == 4 and col_size == 56
        r = kinds.index(WP.TBLIDX)
        idx_cells = plan.pool[plan.records[r, 4]:plan.records[r, 4] + plan.records[r, 1]].tolist()
        n_rows = 1 << plan.k
        assert [cols[c // n_rows][c % n_rows] for c in idx_cells] == [1, 2, 2, 3], "the index kind across table columns"
        r = kinds.index(WP.TABLE)
        src = plan.pool[plan.records[r, 5]:plan.records[r, 5] + plan.records[r, 1]].tolist()
        assert [cols[c // n_rows][c % n_rows] for c in src] == [0, 27, 54, 81]
    if name.startswith("conv_k10"):
        assert circuit.synthesize(img).linear == (607 if circuit.w == 1 else 643)


def test_params_hash_tells_conv_circuits_apart_and_leaves_the_mlp_alone():
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    a, _ = _case_a(1)
    b, _ = _case_a(1)
    assert WP.params_hash(a) == WP.params_hash(b)
    b.fc_b = b.fc_b + 1
    assert WP.params_hash(a) != WP.params_hash(b)
    c = EL.ConvMnistCircuit(logrows=10, image=8, kernel=3, out_channels=2, stride=2, classes=3, lookup_range=(-700, 700), denom=8, decomp_base=32)
    c.kernels, c.fc_w, c.fc_b = a.kernels, a.fc_w, a.fc_b
    assert WP.params_hash(a) != WP.params_hash(c), "the table values are part of the identity"
    assert WP.params_hash(_mlp(9, 2)[0]).hex() == WP.peek(WP.record_plan(_mlp(9, 2)[0]).to_bytes())["param_hash"].hex()


def _assert_pinned(circuit, pin):
    from ezkl_amd import witness_plan as WP
    records, sha, param_hash = pin
    plan = WP.record_plan(circuit)
    blob = plan.to_bytes()
    assert plan.n_records == records
    assert hashlib.sha256(blob).hexdigest() == sha
    assert WP.params_hash(circuit).hex()[:16] == param_hash == WP.peek(blob)["param_hash"].hex()[:16]
    return blob


@pytest.mark.parametrize("name", list(MLP_PINS))
def test_mlp_plans_keep_their_bytes(name):
    from ezkl_amd import witness_plan as WP
    assert set(MLP_PINS) == set(MLP_CASES)
    blob = _assert_pinned(MLP_CASES[name]()[0], MLP_PINS[name])
    assert WP.VERSION == 1 and WP.peek(blob)["n_tables"] == 0 and WP.peek(blob)["n_table_values"] == 0
    assert WP.WitnessPlan.from_bytes(blob).tables == []


@pytest.mark.parametrize("name", list(CONV_PINS))
def test_conv_plans_keep_their_bytes(name):
    _assert_pinned(CASES[name]()[0], CONV_PINS[name])


def _conv_records(plan, kind):
    return [r for r in plan.records.tolist() if r[0] == kind]


def test_records_follow_dependence_levels_not_the_image():
    """every conv dot in ONE dot record, every conv bias addition in ONE add record, and as many records for the 28 x 28 image at k = 17
    as for the 8 x 8 one at k = 10 (the latest-fit rule of the MLP path makes 77 records of the small one's conv + ReLU part, 1751 of
    the large one's: one per alternation of dot and add)"""
    from ezkl_amd import witness_plan as WP
    (a, _), (c, _) = _case_a(1), _case_c()
    pa, pc = WP.record_plan(a), WP.record_plan(c)
    for circuit, plan in ((a, pa), (c, pc)):
        dots, adds = _conv_records(plan, WP.DOT), _conv_records(plan, WP.ADD)
        n_conv = circuit.oc * circuit.slides ** 2
        assert dots[0][1] == n_conv == circuit.length and dots[0][3] == circuit.kernel ** 2, "all conv dots in the first dot record"
        assert adds[0][1] == n_conv, "all conv bias additions in the first add record"
        assert dots[-1][1] == circuit.classes and adds[-1][1] == circuit.classes
    assert pa.n_records == pc.n_records
    assert pa.n_records <= 40
    assert pc.n_ops > 1700 > pa.n_ops                            # (the layout-op calls do grow: one per conv dot, one per bias addition, ...)


def _case_b_out_of_range(w=1):
    return _case_b(w, levels=(3, 2, 1, 4))


def test_lookup_input_outside_the_table_raises():
    from ezkl_amd import witness_plan as WP
    circuit, img = _case_b_out_of_range()
    with pytest.raises(AssertionError, match="lookup input 108 outside the table range"):
        circuit.witness(img)
    plan = WP.record_plan(circuit)
    with pytest.raises(AssertionError, match=r"lookup input.*outside the table range \(nonlinearity record (\d+), element 3\)") as e:
        WP.run_plan_host(plan, img.reshape(-1))
    kinds = plan.records[:, 0].tolist()
    assert "record %d," % kinds.index(WP.TABLE) in str(e.value)


# ---- hand-built plans: one INPUT record, then one TABLE and one TBLIDX record on the inputs ----------------------------------------------
LO, HI, COL = -11, 9, 4


def _div4(x):
    return (abs(x) + 2) // 4 * (1 if x >= 0 else -1)           # rounds half away from zero


def _hand_plan(n_inputs, tables=None, values=None, table_index=0, kinds=None, k=4):
    """column 0 = the inputs, column 1 + j = the j-th of `kinds` (default: TABLE then TBLIDX) applied to them, on rows 0 .. n_inputs - 1;
    the outputs are column 1"""
    from ezkl_amd import witness_plan as WP
    kinds = (WP.TABLE, WP.TBLIDX) if kinds is None else kinds
    n, m = 1 << k, n_inputs
    col = lambda c: [c * n + i for i in range(m)]
    pool = col(0) + list(range(m))
    records = [[WP.INPUT, m, 0, 0, 0, m, 0, 0]]
    for j, kind in enumerate(kinds):
        records.append([kind, m, table_index, 0, len(pool), 0, 0, 0])
        pool += col(1 + j)
    if tables is None:
        tables, values = [(LO, HI - LO + 1, COL, 0)], [_div4(x) for x in range(LO, HI + 1)]
    return WP.WitnessPlan(k, 1 + len(kinds), m, [], [], records, col(1), pool, (1 + len(kinds)) * m, 1 + len(kinds), b"\0" * 32, tables, values)


HAND_INPUTS = [LO, LO + 1, -1, 0, 1, HI, -6, -7, 6]
HAND_BAD = [([0, LO - 1, 1], 1), ([HI + 1, 0, 0], 0), ([0, 0, 1 << 40, -(1 << 40)], 2), ([1, -(1 << 40), LO - 5], 1), ([0, 0, 0, 0, 1 << 62], 4),
            ([-(1 << 62), 1 << 62], 0)]


def test_hand_built_lookup_plans():
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    assert _div4(-6) == _div4(-7) == -2 and _div4(6) == 2 and COL < HI - LO + 1
    plan = _hand_plan(len(HAND_INPUTS)).validate()
    assert WP.WitnessPlan.from_bytes(plan.to_bytes()) == plan
    cols, outs = WP.run_plan_host(plan, HAND_INPUTS)
    m = len(HAND_INPUTS)
    assert cols[0][:m] == [x % EL.R for x in HAND_INPUTS]
    assert cols[1][:m] == outs == [_div4(x) % EL.R for x in HAND_INPUTS]
    assert cols[2][:m] == [(x - LO) // COL for x in HAND_INPUTS]
    assert any(v > EL.R // 2 for v in outs) and max(cols[2]) == (HI - LO) // COL == 5
    assert all(not any(col[m:]) for col in cols)
    for xs, first in HAND_BAD:
        with pytest.raises(AssertionError, match=r"lookup input outside the table range \(nonlinearity record 1, element %d\)" % first):
            WP.run_plan_host(_hand_plan(len(xs)), xs)
    # the index kind alone fails by the same rule
    q = _hand_plan(3, kinds=(WP.TBLIDX,))
    assert WP.run_plan_host(q, [LO, 0, HI])[1] == [0, 2, 5]
    with pytest.raises(AssertionError, match=r"lookup input outside the table range \(nonlinearity_index record 1, element 2\)"):
        WP.run_plan_host(q, [LO, 0, HI + 1])


def test_recorder_refuses_a_table_beyond_int64():
    from ezkl_amd import witness_plan as WP
    circuit, _ = _case_b(1)
    table = circuit.gc.base.static_tables["div_4"]
    table.f = lambda x: x << 70
    with pytest.raises(WP.PlanError, match="a lookup table value beyond int64"):
        WP.record_plan(circuit)


def test_base_region_still_refuses_the_lookup_and_unknown_circuits():
    """the lookup-aware recording is LookupRecordingRegion's: the MLP recorder's region refuses the op by name, and the expressions of a
    lookup do not record on it"""
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    circuit, _ = _case_b(1)
    reg = WP.RecordingRegion(circuit.gc)
    with pytest.raises(WP.PlanError, match="nonlinearity"):
        reg.nonlinearity([], "div_4")
    cell = reg.assign(reg.inputs[0], [EL.Val(WP._Input(0))])[0]
    with pytest.raises(WP.PlanError, match="does not cover"):
        reg.assign(reg.inputs[1], [EL.Val((cell.v - (-100)) // 56)])
    with pytest.raises(WP.PlanError, match="SumProdCircuit"):
        WP.record_plan(EL.SumProdCircuit(8, 1, 400))
    # on the lookup region: an index without the lookup beside it, and a lookup without the range assertion, are refused
    reg = WP.LookupRecordingRegion(circuit.gc)
    cell = reg.assign(reg.inputs[0], [EL.Val(WP._Input(0))])[0]
    with pytest.raises(WP.PlanError, match="a table-column index without its lookup"):
        reg.assign(reg.inputs[1], [EL.Val((cell.v - (-100)) // 56)])
    with pytest.raises(WP.PlanError, match="without the layout's range assertion"):
        reg.assign(reg.output, [EL.Val(reg.base.static_tables["div_4"].f(cell.v))])


def _bad_table_plans():
    """(what both validators must say, plan)"""
    good = _hand_plan(3)
    n = HI - LO + 1
    vals = [_div4(x) for x in range(LO, HI + 1)]
    out = [("lookup table index out of range", _hand_plan(3, table_index=1)),
           ("lookup table index out of range", _hand_plan(3, tables=[], values=[])),
           ("bad lookup table shape", _hand_plan(3, tables=[(LO, 0, COL, 0)], values=vals)),
           ("bad lookup table shape", _hand_plan(3, tables=[(LO, n, 0, 0)], values=vals)),
           ("bad lookup table shape", _hand_plan(3, tables=[((1 << 31) - n + 1, n, COL, 0)], values=vals)),
           ("runs past the table values", _hand_plan(3, tables=[(LO, n, COL, 1)], values=vals)),
           ("runs past the table values", _hand_plan(3, tables=[(LO, n + 1, COL, 0)], values=vals)),
           ("runs past the table values", _hand_plan(3, tables=[(LO, n, COL, 0xffffffff)], values=vals)),
           ("runs past the table values", _hand_plan(3, tables=[(LO, n, COL, 0), (0, 2, 1, n - 1)], values=vals))]
    q = _hand_plan(3)                                             # the lookup reads the cells that only the LATER record writes
    q.records = q.records.copy()
    q.records[1, 5] = q.records[2, 4]
    out.append(("read before", q))
    q = _hand_plan(3)                                             # the index record reads its own destinations
    q.records = q.records.copy()
    q.records[2, 5] = q.records[2, 4]
    out.append(("read before", q))
    return good, out


def test_validators_refuse_bad_table_sections_with_the_same_words():
    import ctypes as C
    from ezkl_amd import native, witness_plan as WP
    L = native.load()
    check = lambda blob: L.ezkl_prover_witness_plan_check(blob, C.c_size_t(len(blob)))
    good, bad = _bad_table_plans()
    WP.validate(good)
    assert check(good.to_bytes()) == 0
    n = HI - LO + 1
    edge = _hand_plan(3, tables=[((1 << 31) - n, n, COL, 0)], values=[0] * n)          # lo + n - 1 = 2^31 - 1 exactly
    WP.validate(edge)
    assert check(edge.to_bytes()) == 0
    for what, q in bad:
        with pytest.raises(WP.PlanError, match=what) as e:
            WP.validate(q)
        with pytest.raises(WP.PlanError, match=what):
            WP.run_plan_host(q, [0, 0, 0])
        blob = q.to_bytes()
        assert check(blob) == -3, what
        said = L.ezkl_prover_last_error().decode()
        assert what in said, (what, said)
        if what != "read before":                                 # the new refusals: word for word
            assert str(e.value) == said, (str(e.value), said)
    # the blob length includes the table section exactly
    blob = good.to_bytes()
    for other in (blob[:-8], blob + b"\0" * 8, blob[:-1]):
        with pytest.raises(WP.PlanError, match="bytes"):
            WP.WitnessPlan.from_bytes(other)
        assert check(other) == -3 and "bytes" in L.ezkl_prover_last_error().decode()
    more = bytearray(blob); more[52:56] = (n + 1).to_bytes(4, "little")               # header word 13: one more value than the blob holds
    with pytest.raises(WP.PlanError, match="bytes"):
        WP.WitnessPlan.from_bytes(bytes(more))
    assert check(bytes(more)) == -3 and "bytes" in L.ezkl_prover_last_error().decode()
    # the recorded conv plans pass the C++ check as they pass the Python one
    for name in ("conv_k10_w2", "conv_k6_w1_4_blocks_4_table_columns"):
        assert check(WP.record_plan(CASES[name]()[0]).to_bytes()) == 0
