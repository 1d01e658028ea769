"""The scatter, complement and one-hot kernels (csrc/witness.hip: wit_scatter_lds_kernel and wit_compl_lds_kernel up to SCATTER_TILE cells, the
fill / mark / store and fill / mark / count / offsets / compact launches above it, the ONEHOT branch of wit_elem_kernel) on the device: every
synthetic plan of tests/witness_synth_scatter.py twice into the same dirty columns, the device columns, the status words and the error text
against the closed form; a scatter with two indices outside its dimension left unwritten while its neighbours are written; all elements onto
one target the same on every run; and ScatterGatherCircuit recorded, run and proved from the device-made columns."""
import re

import numpy as np
import pytest

import witness_synth_scatter as T

pytestmark = pytest.mark.gpu
SEEDS = (1, 2)
# logrows, inner columns, capacity.  The layout also fits k = 9 (483 cells of the linear coordinate, 108 rows of dynamic tables), in more advice
# columns: as for the pool classifier, the quotient kernel of the wider constraint system takes longer to compile there (5.5 s at k = 9
# against 2 - 4 s at k = 10, measured on that circuit): k = 10 is the smallest k that keeps the case to a few seconds
SHAPE = (10, 2, 6000)


def _assert_columns(cols, case):
    from ezkl_amd import ezkl_layout as EL
    k = case.plan.k
    got = {}
    for c, want in enumerate(EL.cols_to_mont(case.columns())):
        got[c] = cols[c].to_numpy(shape=(1 << k, 4))
        assert got[c].tobytes() == want.tobytes(), "column %d differs on rows %s" % (c, (got[c] != want).any(1).nonzero()[0][:8].tolist())
    for cell in case.unwritten:
        assert not got[cell >> k][cell & ((1 << k) - 1)].any(), "a refused record wrote cell %d" % cell
    return got


def _run(B, dev, cols, case):
    from ezkl_amd import witness_plan as WP
    plan = case.plan
    if case.refused:
        ri, el = case.refused[0]
        kind = int(plan.records[ri, 0])
        words = "%s (%s record %d, element %d; %d cells in all)" % ({WP.SCATTER: WP.SCATTER_ERROR, WP.ONEHOT: WP.ONEHOT_ERROR}[kind], WP.kind_name(kind), ri, el, len(case.refused))
        with pytest.raises(B.WitnessError, match=re.escape(words)):
            dev.run(case.x, columns=cols)
        assert dev.last["failed"] == len(case.refused) and dev.last["first"] == case.refused[0]
    else:
        _, outs = dev.run(case.x, columns=cols)
        assert outs == case.outputs() and dev.last["failed"] == 0
    assert dev.last["cells_written"] == plan.n_cells - len(case.unwritten)
    return _assert_columns(cols, case)


@pytest.mark.parametrize("name", list(T.CASES))
def test_device_columns_equal_the_closed_form(hip, name):
    from ezkl_amd import backend as B
    cols, devs = None, []
    try:
        for seed in SEEDS:                                           # other values into the columns the first run left dirty
            case = T.CASES[name](seed)
            devs.append(B.WitnessPlan(case.plan.to_bytes()))
            cols = cols or devs[-1].alloc_columns()
            _run(B, devs[-1], cols, case)
    finally:
        for c in cols or []:
            c.free()
        for dev in devs:
            dev.free()


def test_a_complement_of_more_tiles_than_lanes(hip):
    """256 tiles and one position: wit_compl_offsets_kernel carries its running total into a second round"""
    from ezkl_amd import backend as B
    case = T.offsets_case(1)
    dev = B.WitnessPlan(case.plan.to_bytes())
    cols = dev.alloc_columns()
    try:
        _run(B, dev, cols, case)
    finally:
        for c in cols:
            c.free()
        dev.free()


@pytest.mark.parametrize("n", [100, T.TILE + 1])
def test_a_scatter_with_indices_outside_its_dimension_is_left_unwritten_and_the_next_run_is_clean(hip, n):
    from ezkl_amd import backend as B, witness_plan as WP
    bad = T.failing_case(n, True, seed=7)
    dev = B.WitnessPlan(bad.plan.to_bytes())
    cols = dev.alloc_columns()
    try:
        _run(B, dev, cols, T.failing_case(n, False, seed=6))
        assert bad.refused == [(6, e) for e in T.BAD_AT] and len(bad.unwritten) == n
        _run(B, dev, cols, bad)                                      # 2 offending elements, the first of them named; n cells left zero, the two neighbours written
        with pytest.raises(AssertionError, match=re.escape("%s (scatter record 6, element %d)" % (WP.SCATTER_ERROR, T.BAD_AT[0]))):
            WP.run_plan_host(bad.plan, bad.x)                        # the interpreter's words
        _run(B, dev, cols, T.failing_case(n, False, seed=8))
    finally:
        for c in cols:
            c.free()
        dev.free()


@pytest.mark.parametrize("n", [257, T.TILE + 1])
def test_all_elements_onto_one_target_give_the_same_columns_on_every_run(hip, n):
    """n + 3 lanes race for one winner word, in LDS and in the scratch: the greatest element wins whatever the order they arrive in"""
    from ezkl_amd import backend as B
    case = T.scatter_case(n, 5, contents=["onto-one"])
    dev = B.WitnessPlan(case.plan.to_bytes())
    cols = dev.alloc_columns()
    try:
        first = _run(B, dev, cols, case)
        second = _run(B, dev, cols, case)
        assert all(first[c].tobytes() == second[c].tobytes() for c in first)
    finally:
        for c in cols:
            c.free()
        dev.free()


def test_create_proof_from_device_columns_writes_the_same_bytes(hip):
    """ScatterGatherCircuit at k = 10: the device columns are the host layout's, the proof from them is the proof from the host's (same
    seed), made under CheckMode SAFE -- the verifier accepts it"""
    from ezkl_amd import backend as B, ezkl_layout as EL, native as NV, witness_plan as WP
    from test_gpu_witness import _assert_columns as assert_layout, _keygen
    from test_witness_plan_scatter_cpu import inputs
    circuit = lambda: EL.ScatterGatherCircuit(*SHAPE)
    c = circuit()
    x, x2 = inputs(c, 11), inputs(c, 12)
    adv, inst = c.witness(x)
    assert [EL.signed(v) for v in inst[0]] == c.model(x)
    host = EL.cols_to_mont(adv)
    pk, bg, bgl, _ = _keygen(circuit(), x)
    g2, s_g2 = NV.g2_mul_generator(1), NV.g2_mul_generator(0x5eed)
    plan = WP.record_plan(circuit())
    dev = B.WitnessPlan(plan.to_bytes())
    cols, outs = dev.run(x)
    try:
        assert_layout(B, c, x, cols, outs)
        kinds = plan.records[:, 0].tolist()
        assert dev.last["cells_written"] == plan.n_cells and dev.last["failed"] == 0
        assert (kinds.count(WP.SCATTER), kinds.count(WP.COMPLEMENT), kinds.count(WP.ONEHOT)) == (1, 1, 1)
        ref = NV.create_proof(pk, bg, bgl, host, seed=7, instances=inst, check_mode="SAFE", g2=g2, s_g2=s_g2)
        assert NV.create_proof(pk, bg, bgl, list(cols), seed=7, instances=inst, check_mode="SAFE", g2=g2, s_g2=s_g2) == ref
        assert NV.verify_proof(pk, g2, s_g2, ref, inst)
        _, outs2 = dev.run(x2, columns=cols)                          # other inputs into the same columns
        assert_layout(B, circuit(), x2, cols, outs2)
    finally:
        for col in cols:
            col.free()
        dev.free(); bg.free(); bgl.free()
