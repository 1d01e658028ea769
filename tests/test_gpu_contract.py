"""CONTRACT records on the device (csrc/witness.hip wit_contract_gather_kernel, wit_contract_gemm_kernel): hand-built plans against a direct
Python-integer contraction reduced mod r -- never the host interpreter --, the failure, and the attention head under the contract claim."""
import json
import re

import numpy as np
import pytest

from test_contract_cpu import M31, PATTERNS, SHAPES, contract_plan, expected_columns, operands

pytestmark = pytest.mark.gpu


def _run(B, plan, x, want, twice=False):
    """the plan on the device, phase by phase, into columns that start dirty: every column byte-equal to `want` (canonical integers)"""
    from ezkl_amd import ezkl_layout as EL
    dev = B.WitnessPlan(plan.to_bytes())
    cols = dev.alloc_columns()
    try:
        for _ in range(2 if twice else 1):
            written = 0
            for phase in range(plan.n_phases):
                dev.run(x if phase == 0 else None, columns=cols, **({} if plan.n_phases == 1 else dict(phase=phase, challenges=[])))
                written += dev.last["cells_written"]
            assert written == plan.n_cells and dev.last["failed"] == 0
            for i, (d, r) in enumerate(zip(cols, EL.cols_to_mont(want))):
                got = d.to_numpy(shape=(1 << plan.k, 4))
                assert got.tobytes() == r.tobytes(), "column %d: rows %s differ" % (i, np.nonzero((got != r).any(1))[0][:8].tolist())
    finally:
        for col in cols:
            col.free()
        dev.free()


# one record at every shape; a record in phase 1 over phase-0 cells; a smaller record after a larger one, in scratch the first filled further
@pytest.mark.parametrize("shapes,phase", [([s], 0) for s in SHAPES] + [([(65, 17, 5)], 1), ([(65, 33, 63), (3, 5, 2)], 0)])
def test_plans_equal_the_integer_contraction(hip, shapes, phase):
    from ezkl_amd import backend as B
    for pattern in PATTERNS:
        plan, layout = contract_plan(shapes, repeated=pattern == "repeated", phase=phase)
        x = sum((v for s in shapes for v in operands(*s, pattern, seed=s[1])), [])
        _run(B, plan, x, expected_columns(plan, layout, shapes, x), twice=pattern == "max")


@pytest.mark.parametrize("where", ["first of a", "last of b"])
def test_an_operand_outside_the_range_is_reported_and_the_record_writes_nothing(hip, where):
    from ezkl_amd import backend as B, witness_plan as WP
    m, kd, n = 65, 33, 63
    plan, layout = contract_plan([(m, kd, n)])
    x = sum(operands(m, kd, n, "max"), [])
    at, value = (0, 1 << 31) if where == "first of a" else (m * kd + kd * n - 1, -(1 << 31))
    x[at] = value
    words = "einsum operand outside the exact-product range (contract record 1, element %d" % at
    dev = B.WitnessPlan(plan.to_bytes())
    cols = dev.alloc_columns()
    try:
        with pytest.raises(B.WitnessError, match=re.escape(words + "; 1 operand reads in all)")):
            dev.run(x, columns=cols)
        assert dev.last["first"] == (1, at) and dev.last["failed"] == 1 and dev.last["cells_written"] == len(x), "only the inputs were placed"
        assert not any(cols[cell >> plan.k].to_numpy(shape=(1 << plan.k, 4)).any() for cell in layout[0][2][::1 << plan.k]), "a destination column was written"
        with pytest.raises(AssertionError, match=re.escape(words + ")")):
            WP.run_plan_host(plan, x)
        x[at] = M31 if value > 0 else -M31                          # the bound itself passes, on the same plan and columns
        dev.run(x, columns=cols)
        assert dev.last["cells_written"] == plan.n_cells
    finally:
        for col in cols:
            col.free()
        dev.free()


def test_the_attention_head_writes_the_dot_plans_columns_and_proof(hip):
    from ezkl_amd import backend as B, ezkl_layout as EL, native as NV, plonk as P
    R = EL.R
    chal = [0x1234567890abcdef1234567890abcdef % R, 0xfedcba0987654321]
    built = {claim: EL.AttentionHeadCircuit(10, 4, 4, 2, capacity=6 << 10, einsum_claim=claim).build(gpu=B, synthesis="device") for claim in ("dot", "contract")}
    try:
        dot, con = built["dot"], built["contract"]
        cs = dot["cs"]
        cols = {claim: {**b["advice"](0, []), **b["advice"](1, chal)} for claim, b in built.items()}
        for i in range(cs.n_advice):
            assert cols["contract"][i].to_numpy(shape=(cs.n, 4)).tobytes() == cols["dot"][i].to_numpy(shape=(cs.n, 4)).tobytes(), "advice column %d differs" % i
        s = 0x1234567890abcdef1234567890abcdef % R
        gb, glb = B.gen_srs(10, s)
        pk = NV.NativeProvingKey(NV.NativeCircuit(cs), gb, EL.cols_to_mont(dot["fixed"], B), dot["copies"])
        proofs = [NV.create_proof(pk, gb, glb, b["advice"], rng=P.Rng(5), instances=b["instances"], device_columns=b["device_columns"]) for b in (dot, con)]
        assert proofs[0] == proofs[1] and NV.verify_proof(pk, NV.g2_mul_generator(1), NV.g2_mul_generator(s), proofs[1], con["instances"])
        gb.free(); glb.free()
    finally:
        for b in built.values():
            b["witness"].free()


def test_a_description_with_the_field_runs_through_execute(hip, tmp_path, monkeypatch):
    from ezkl_amd import ezkl_layout as EL, execute as X, witness_plan as WP
    monkeypatch.setenv("ENABLE_HIP_GPU", "1")
    monkeypatch.setenv("HIP_SMALL_K", "4")
    c = EL.AttentionHeadCircuit(10, 4, 4, 2, capacity=6 << 10, einsum_claim="contract")
    j = X.describe(c)
    assert j["einsum_claim"] == "contract"
    f = {name: str(tmp_path / name) for name in ("circuit.json", "kzg.srs", "vk.key", "pk.key", "w.json", "proof.json")}
    open(f["circuit.json"], "w").write(json.dumps(j))
    X.gen_srs(f["kzg.srs"], 10, secret=0x5eed)
    X.setup(f["circuit.json"], f["kzg.srs"], f["vk.key"], f["pk.key"])
    plan = WP.WitnessPlan.from_bytes(open(f["pk.key"] + ".wplan", "rb").read())
    assert plan.version == 2 and plan.param_hash == WP.params_hash(c) and (plan.records[:, 0] == WP.CONTRACT).sum() == 5
    X.gen_witness(f["circuit.json"], {"input_data": [[float(v) for v in c.default_inputs()]]}, output=f["w.json"], synthesis="device", pk_path=f["pk.key"])
    how = {}
    X.prove(f["w.json"], f["circuit.json"], f["pk.key"], f["proof.json"], f["kzg.srs"], seed=31, synthesis="device", report=how)
    assert how["path"] == "device" and X.verify(f["proof.json"], f["circuit.json"], f["vk.key"], f["kzg.srs"])
