"""Witness synthesis of the conv family on the device (csrc/witness.hip: the static-lookup kinds, plans recorded from the circuit's own
`layout`): the columns the kernels write are byte-equal to cols_to_mont(circuit.witness(img)), hand-built lookup plans agree with the host
interpreter at the table ends and on the negative side, a lookup input outside its table is reported with the record and element the
host interpreter names and the process goes on, and create_proof / the mock prover take the device-made columns as they take the host's."""
import numpy as np
import pytest

from test_gpu_witness import _assert_columns, _keygen
from test_witness_plan_lookup_cpu import CASES, HAND_BAD, HAND_INPUTS, _case_a, _case_b, _case_b_out_of_range, _case_c, _hand_plan

pytestmark = pytest.mark.gpu


def _run(B, circuit, img):
    from ezkl_amd import witness_plan as WP
    plan = WP.record_plan(circuit)
    dev = B.WitnessPlan(plan.to_bytes())
    cols, outs = dev.run(img.reshape(-1))
    return plan, dev, cols, outs, dev.last


@pytest.mark.parametrize("name", list(CASES))
def test_device_columns_equal_the_conv_layout(hip, name):
    from ezkl_amd import backend as B
    circuit, img = CASES[name]()
    plan, dev, cols, outs, last = _run(B, circuit, img)
    try:
        _assert_columns(B, circuit, img, cols, outs)
        assert last["cells_written"] == plan.n_cells == dev.n_cells and last["failed"] == 0
        assert dev.n_records == plan.n_records and dev.n_ops == plan.n_ops
        # fills of the columns and of the status words, one launch per record, the output gather
        assert plan.n_records <= last["launches"] <= plan.n_records + plan.n_advice + 2 <= 4 * plan.n_ops
        assert last["device_ms"] > 0
        # the same plan, another image, the same columns (dirty from the first run: the run zero-fills them)
        img2 = (img + 1) % 4
        cols2, outs2 = dev.run(img2.reshape(-1), columns=cols)
        assert cols2 is cols
        _assert_columns(B, circuit, img2, cols, outs2)
    finally:
        for c in cols:
            c.free()
        dev.free()


def test_hand_built_lookup_plans_on_the_device(hip):
    from ezkl_amd import backend as B, ezkl_layout as EL, witness_plan as WP
    plan = _hand_plan(len(HAND_INPUTS))
    ref_cols, ref_outs = WP.run_plan_host(plan, HAND_INPUTS)
    dev = B.WitnessPlan(plan.to_bytes())
    cols = dev.alloc_columns()
    try:
        _, outs = dev.run(HAND_INPUTS, columns=cols)
        assert outs == ref_outs and dev.last["failed"] == 0 and dev.last["cells_written"] == plan.n_cells
        for d, r in zip(cols, EL.cols_to_mont(ref_cols)):
            assert d.to_numpy(shape=(1 << plan.k, 4)).tobytes() == r.tobytes()
    finally:
        for c in cols:
            c.free()
        dev.free()
    for xs, first in HAND_BAD:                                    # reported, not a fault: the smallest failing (record, element), as on the host
        dev = B.WitnessPlan(_hand_plan(len(xs)).to_bytes())
        try:
            with pytest.raises(B.WitnessError, match=r"lookup input outside the table range \(nonlinearity record 1, element %d;" % first):
                dev.run(xs)
            assert dev.last["first"] == (1, first) and dev.last["failed"] >= 2          # the lookup lane and the index lane of each bad input
        finally:
            dev.free()
    q = _hand_plan(3, kinds=(WP.TBLIDX,))
    dev = B.WitnessPlan(q.to_bytes())
    try:
        with pytest.raises(B.WitnessError, match=r"lookup input outside the table range \(nonlinearity_index record 1, element 2;"):
            dev.run([-11, 0, 10])
        cols, outs = dev.run([-11, 0, 9])
        assert outs == [0, 2, 5]
        for c in cols:
            c.free()
    finally:
        dev.free()


def test_lookup_input_outside_the_table_is_reported_and_the_process_goes_on(hip):
    from ezkl_amd import backend as B, witness_plan as WP
    circuit, bad = _case_b_out_of_range()
    _, img = _case_b(1)
    plan = WP.record_plan(circuit)
    dev = B.WitnessPlan(plan.to_bytes())
    cols = dev.alloc_columns()
    try:
        with pytest.raises(B.WitnessError, match="lookup input outside the table range.*nonlinearity record") as e:
            dev.run(bad.reshape(-1), columns=cols)
        assert dev.last["failed"] >= 1 and dev.last["cells_written"] < plan.n_cells
        rec, elem = dev.last["first"]
        assert plan.records[rec, 0] == WP.TABLE and elem == 3 and "record %d, element %d" % (rec, elem) in str(e.value)
        with pytest.raises(AssertionError, match="lookup input.*outside the table range.*record %d, element %d" % (rec, elem)):
            WP.run_plan_host(plan, bad.reshape(-1))               # the host interpreter names the same cell
        # the next valid run in the same process, into the same columns, is correct
        _, outs = dev.run(img.reshape(-1), columns=cols)
        _assert_columns(B, circuit, img, cols, outs)
        assert dev.last["failed"] == 0 and dev.last["cells_written"] == plan.n_cells
    finally:
        for c in cols:
            c.free()
        dev.free()


@pytest.mark.parametrize("case", ["conv_k10_w1", "conv_mnist_k17"])
def test_create_proof_from_device_columns_writes_the_same_bytes(hip, case):
    """keygen as tests/test_gpu_witness.py does it; the proof from the device-made columns is the proof from the host's (same seed), under
    CheckMode SAFE; at k = 10 the mock prover reports nothing on the device-made columns"""
    from ezkl_amd import backend as B, ezkl_layout as EL, native as NV
    circuit, img = (_case_a(1) if case == "conv_k10_w1" else _case_c())
    adv, inst = circuit.witness(img)
    host = EL.cols_to_mont(adv)
    pk, bg, bgl, (cs, fixed, copies) = _keygen(circuit, img)
    g2, s_g2 = NV.g2_mul_generator(1), NV.g2_mul_generator(0x5eed)
    plan, dev, cols, outs, _ = _run(B, circuit, img)
    try:
        assert [outs] == inst
        ref = NV.create_proof(pk, bg, bgl, host, seed=7, instances=inst, check_mode="SAFE", g2=g2, s_g2=s_g2)
        assert NV.create_proof(pk, bg, bgl, list(cols), seed=7, instances=inst, check_mode="SAFE", g2=g2, s_g2=s_g2) == ref
        if case == "conv_k10_w1":
            n = 1 << circuit.k
            records, totals = NV.mock(cs, EL.cols_to_mont(fixed, B), copies, [c.to_numpy(shape=(n, 4)) for c in cols], instances=[outs])
            assert list(totals) == [0, 0, 0] and not records
    finally:
        for c in cols:
            c.free()
        dev.free(); bg.free(); bgl.free()
