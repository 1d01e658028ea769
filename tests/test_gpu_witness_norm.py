"""The RECIP and ISQRT branches of wit_elem_kernel (csrc/witness.hip) on the device: every synthetic plan of tests/witness_synth_norm.py twice
into the same dirty columns, the device columns, the status words and the error text against the closed form; operands beyond the range
refused at the wave edge while their neighbours are written; and NormCircuit -- softmax and layer norm -- recorded, run and proved from
the device-made columns."""
import re

import pytest

import witness_synth_norm as T

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
        assert not got[cell >> k][cell & ((1 << k) - 1)].any(), "a refused lane wrote cell %d" % cell


def _run(B, dev, cols, case, words=None):
    from ezkl_amd import witness_plan as WP
    plan = case.plan
    if case.refused:
        ri, el = case.refused[0]
        text = "%s (%s record %d, element %d; %d cells in all)" % (words, WP.kind_name(int(plan.records[ri, 0])), ri, el, len(case.refused))
        with pytest.raises(B.WitnessError, match=re.escape(text)):
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


@pytest.mark.parametrize("kind,scale", [("recip", s) for s in T.RECIP_SCALES] + [("sqrt", s) for s in T.SQRT_SCALES])
def test_operands_beyond_the_range_are_refused_and_the_next_run_is_clean(hip, kind, scale):
    """elements 63 and 64 of 130 -- the last lane of a wave and the first of the next: beyond 62 bits, or (sqrt) with T = 2^62 reached by a
    value that fits -- report themselves and leave their cells zero; elements 62 and 65 and every other one are written"""
    from ezkl_amd import backend as B, witness_plan as WP
    kd, words = (WP.RECIP, WP.RECIP_ERROR) if kind == "recip" else (WP.ISQRT, WP.SQRT_ERROR)
    bad = T.failing_case(kd, scale, True, seed=7)
    dev = B.WitnessPlan(bad.plan.to_bytes())
    cols = dev.alloc_columns()
    try:
        _run(B, dev, cols, T.failing_case(kd, scale, False, seed=6))
        assert bad.refused == [(1, e) for e in T.BAD_AT] and len(bad.unwritten) == 2
        _run(B, dev, cols, bad, words)
        with pytest.raises(AssertionError, match=re.escape("%s (%s record 1, element %d)" % (words, kind, T.BAD_AT[0]))):
            WP.run_plan_host(bad.plan, bad.x)                        # the interpreter's words
        _run(B, dev, cols, T.failing_case(kd, scale, False, seed=8))
    finally:
        for c in cols:
            c.free()
        dev.free()


@pytest.mark.parametrize("variant", ["softmax", "layer_norm"])
def test_create_proof_from_device_columns_writes_the_same_bytes(hip, variant):
    """NormCircuit at k = 9: the device columns are the host layout's, the proof from them is the proof from the host's (same seed),
    made under CheckMode SAFE -- the verifier accepts it"""
    from ezkl_amd import backend as B, ezkl_layout as EL, native as NV, witness_plan as WP
    from test_gpu_witness import _assert_columns as assert_layout, _keygen
    from test_norm_layout_cpu import circuit, inputs
    x = inputs(11)
    c = circuit(variant)
    adv, inst = c.witness(x)
    host = EL.cols_to_mont(adv)
    pk, bg, bgl, _ = _keygen(circuit(variant), x)
    g2, s_g2 = NV.g2_mul_generator(1), NV.g2_mul_generator(0x5eed)
    plan = WP.record_plan(circuit(variant))
    dev = B.WitnessPlan(plan.to_bytes())
    cols, outs = dev.run(x)
    try:
        assert_layout(B, c, x, cols, outs)
        kinds = set(plan.records[:, 0].tolist())
        assert dev.last["cells_written"] == plan.n_cells and dev.last["failed"] == 0 and WP.RECIP in kinds and (WP.ISQRT in kinds) == (variant == "layer_norm")
        ref = NV.create_proof(pk, bg, bgl, host, seed=7, instances=inst, check_mode="SAFE", g2=g2, s_g2=s_g2)
        assert NV.create_proof(pk, bg, bgl, list(cols), seed=7, instances=inst, check_mode="SAFE", g2=g2, s_g2=s_g2) == ref
        assert NV.verify_proof(pk, g2, s_g2, ref, inst)
        x2 = inputs(12)                                               # other inputs into the same columns
        _, outs2 = dev.run(x2, columns=cols)
        assert_layout(B, circuit(variant), x2, cols, outs2)
    finally:
        for col in cols:
            col.free()
        dev.free(); bg.free(); bgl.free()
