"""The arg-extremum kernels (csrc/witness.hip: wit_argext_wave_kernel for segments up to a wave, wit_argext_group_kernel up to a chunk and
per chunk above it, wit_argext_final_kernel over the chunk slots) on the device: every synthetic plan of tests/witness_synth_pool.py twice
into the same dirty columns, the device columns, the status words and the error text against the closed form; a segment with sources beyond
62 bits left unwritten while its neighbours are written; and PoolClassifierCircuit -- max and sum pooling -- recorded, run and proved from
the device-made columns."""
import re

import numpy as np
import pytest

import witness_synth_pool as T

pytestmark = pytest.mark.gpu
SEEDS = (1, 2)
# logrows, inner columns, capacity.  The layout also fits k = 8 (57 advice columns of the 64 a plan may have) and k = 9 (33), but the quotient
# kernel of so wide a constraint system takes 10 s / 5.5 s to compile against 2 - 4 s at k = 10 (21 columns): the smallest k that keeps a case
# to a few seconds
SHAPE = (10, 2, 4400)


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
        words = "%s (%s record %d, element %d; %d cells in all)" % (WP.ARGEXT_ERROR, WP.kind_name(int(plan.records[ri, 0])), ri, el, len(case.refused))
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


@pytest.mark.parametrize("n", [100, T.CHUNK + 1])
def test_a_segment_with_sources_beyond_62_bits_is_left_unwritten_and_the_next_run_is_clean(hip, n):
    from ezkl_amd import backend as B, witness_plan as WP
    bad = T.failing_case(n, True, seed=7)
    dev = B.WitnessPlan(bad.plan.to_bytes())
    cols = dev.alloc_columns()
    try:
        _run(B, dev, cols, T.failing_case(n, False, seed=6))
        assert bad.refused == [(1, n + e) for e in T.BAD_AT] and len(bad.unwritten) == 1
        _run(B, dev, cols, bad)                                      # 2 offending reads, the first of them named; 1 cell left zero, its two neighbours written
        with pytest.raises(AssertionError, match=re.escape("%s (argext record 1, element %d)" % (WP.ARGEXT_ERROR, n + T.BAD_AT[0]))):
            WP.run_plan_host(bad.plan, bad.x)                        # the interpreter's words
        _run(B, dev, cols, T.failing_case(n, False, seed=8))
    finally:
        for c in cols:
            c.free()
        dev.free()


@pytest.mark.parametrize("pool", ["max", "sum"])
def test_create_proof_from_device_columns_writes_the_same_bytes(hip, pool):
    """PoolClassifierCircuit at k = 10: the device columns are the host layout's, the proof from them is the proof from the host's (same
    seed), made under CheckMode SAFE -- the verifier accepts it"""
    from ezkl_amd import backend as B, ezkl_layout as EL, native as NV, witness_plan as WP
    from test_gpu_witness import _assert_columns as assert_layout, _keygen
    circuit = lambda: EL.PoolClassifierCircuit(*SHAPE, pool=pool)
    rng = np.random.default_rng(11)
    x, x2 = (rng.integers(0, 16, 64).tolist() for _ in range(2))
    c = circuit()
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
        kinds = set(plan.records[:, 0].tolist())
        assert dev.last["cells_written"] == plan.n_cells and dev.last["failed"] == 0
        assert {WP.ARGEXT, WP.SORT} <= kinds and (WP.DIVC in kinds) == (pool == "sum")
        ref = NV.create_proof(pk, bg, bgl, host, seed=7, instances=inst, check_mode="SAFE", g2=g2, s_g2=s_g2)
        assert NV.create_proof(pk, bg, bgl, list(cols), seed=7, instances=inst, check_mode="SAFE", g2=g2, s_g2=s_g2) == ref
        assert NV.verify_proof(pk, g2, s_g2, ref, inst)
        _, outs2 = dev.run(x2, columns=cols)                          # other inputs into the same columns
        assert_layout(B, circuit(), x2, cols, outs2)
    finally:
        for col in cols:
            col.free()
        dev.free(); bg.free(); bgl.free()
