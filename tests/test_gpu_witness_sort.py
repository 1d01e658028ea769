"""The sort kernels (csrc/witness.hip: wit_sort_lds_kernel for segments up to a tile, the tile / global / merge / store launches above
it) on the device: every synthetic plan of tests/witness_synth_sort.py twice into the same dirty columns, the device columns, the status
words and the error text against the closed form; a segment with keys beyond 62 bits refused whole while its neighbours are written;
and SortTopkCircuit recorded, run and proved from the device-made columns."""
import re

import pytest

import witness_synth_sort as T

pytestmark = pytest.mark.gpu
SEEDS = (1, 2)


def _assert_columns(cols, case):
    from ezkl_amd import ezkl_layout as EL
    k = case.plan.k
    got = {}
    for c, want in enumerate(EL.cols_to_mont(case.columns())):
        got[c] = cols[c].to_numpy(shape=(1 << k, 4))
        assert got[c].tobytes() == want.tobytes(), "column %d differs on rows %s" % (c, (got[c] != want).any(1).nonzero()[0][:8].tolist())
    for cell in case.unwritten:
        assert not got[cell >> k][cell & ((1 << k) - 1)].any(), "a refused segment wrote cell %d" % cell


def _run(B, dev, cols, case):
    from ezkl_amd import witness_plan as WP
    plan = case.plan
    if case.refused:
        ri, el = case.refused[0]
        words = "%s (%s record %d, element %d; %d cells in all)" % (WP.SORT_ERROR, WP.kind_name(int(plan.records[ri, 0])), ri, el, len(case.refused))
        with pytest.raises(B.WitnessError, match=re.escape(words)):
            dev.run(case.x, columns=cols)
        assert dev.last["failed"] == len(case.refused) and dev.last["first"] == case.refused[0]
    else:
        _, outs = dev.run(case.x, columns=cols)
        assert outs == case.outputs() and dev.last["failed"] == 0
    assert dev.last["cells_written"] == plan.n_cells - len(case.unwritten)
    _assert_columns(cols, case)


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


@pytest.mark.parametrize("n", [100, T.TILE + 1])
def test_a_segment_with_keys_beyond_62_bits_is_refused_whole_and_the_next_run_is_clean(hip, n):
    from ezkl_amd import backend as B, witness_plan as WP
    bad = T.failing_case(n, True, seed=7)
    dev = B.WitnessPlan(bad.plan.to_bytes())
    cols = dev.alloc_columns()
    try:
        _run(B, dev, cols, T.failing_case(n, False, seed=6))
        sort_ri, arg_ri = [ri for ri, r in enumerate(bad.plan.records.tolist()) if r[0] in (WP.SORT, WP.ARGSORT)]
        assert bad.refused == [(ri, n + e) for ri in (sort_ri, arg_ri) for e in T.BAD_AT] and len(bad.unwritten) == 2 * n
        _run(B, dev, cols, bad)                                      # 6 offending reads, the first of them named; 2 n cells left zero, 4 n written
        with pytest.raises(AssertionError, match=re.escape("%s (sort record %d, element %d)" % (WP.SORT_ERROR, sort_ri, n + T.BAD_AT[0]))):
            WP.run_plan_host(bad.plan, bad.x)                        # the interpreter's words
        _run(B, dev, cols, T.failing_case(n, False, seed=8))
    finally:
        for c in cols:
            c.free()
        dev.free()


@pytest.mark.parametrize("mode", ["unsorted", "largest_index_first"])
def test_create_proof_from_device_columns_writes_the_same_bytes(hip, mode):
    """SortTopkCircuit at k = 9: the device columns are the host layout's, the proof from them is the proof from the host's (same seed),
    made under CheckMode SAFE -- the verifier accepts it"""
    from ezkl_amd import backend as B, ezkl_layout as EL, native as NV, witness_plan as WP
    from test_gpu_witness import _assert_columns as assert_layout, _keygen
    from test_sort_layout_cpu import circuit, inputs
    shape = (9, 2, 13)
    x = inputs(13, 11)
    c = circuit(*shape, mode)
    adv, inst = c.witness(x)
    host = EL.cols_to_mont(adv)
    pk, bg, bgl, _ = _keygen(circuit(*shape, mode), x)
    g2, s_g2 = NV.g2_mul_generator(1), NV.g2_mul_generator(0x5eed)
    plan = WP.record_plan(circuit(*shape, mode))
    dev = B.WitnessPlan(plan.to_bytes())
    cols, outs = dev.run(x)
    try:
        assert_layout(B, c, x, cols, outs)
        assert dev.last["cells_written"] == plan.n_cells and dev.last["failed"] == 0 and {WP.SORT, WP.ARGSORT} <= set(plan.records[:, 0].tolist())
        ref = NV.create_proof(pk, bg, bgl, host, seed=7, instances=inst, check_mode="SAFE", g2=g2, s_g2=s_g2)
        assert NV.create_proof(pk, bg, bgl, list(cols), seed=7, instances=inst, check_mode="SAFE", g2=g2, s_g2=s_g2) == ref
        assert NV.verify_proof(pk, g2, s_g2, ref, inst)
        x2 = inputs(13, 12)                                           # other inputs into the same columns
        _, outs2 = dev.run(x2, columns=cols)
        assert_layout(B, circuit(*shape, mode), x2, cols, outs2)
    finally:
        for col in cols:
            col.free()
        dev.free(); bg.free(); bgl.free()
