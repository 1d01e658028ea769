"""Witness synthesis on the device (csrc/witness.hip through backend.WitnessPlan) against the layout engine: the columns the kernels
write are byte-equal to cols_to_mont(circuit.witness(x)), create_proof takes them where they are (EZKL_COLUMN_DEVICE_FP) and writes the
proof it writes from host columns, `execute.prove(synthesis="device")` writes the bytes of `synthesis="host"`, and a value outside its
decomposition range is reported by name without ending the process."""
import json
import os
import sys

import numpy as np
import pytest

import fixture_k6 as FX
from test_ezkl_circuit import FIXTURE_B, FIXTURE_W
from test_witness_plan_cpu import CASES, _relu_only

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(B, circuit, x):
    """-> (plan, device handle, columns, outputs, counters)"""
    from ezkl_amd import witness_plan as WP
    plan = WP.record_plan(circuit)
    dev = B.WitnessPlan(plan.to_bytes())
    cols, outs = dev.run(x)
    return plan, dev, cols, outs, dev.last


def _assert_columns(B, circuit, x, cols, outs):
    from ezkl_amd import ezkl_layout as EL
    adv, inst = circuit.witness(x)
    ref = EL.cols_to_mont(adv)
    n = 1 << circuit.k
    assert len(cols) == len(ref)
    for c, (d, r) in enumerate(zip(cols, ref)):
        got = d.to_numpy(shape=(n, 4))
        assert got.tobytes() == r.tobytes(), "advice column %d differs on rows %s" % (c, np.nonzero((got != r).any(1))[0][:8].tolist())
    assert [outs] == inst


@pytest.mark.parametrize("name", list(CASES))
def test_device_columns_equal_the_layout_engine(hip, name):
    from ezkl_amd import backend as B
    circuit, x = CASES[name]()
    plan, dev, cols, outs, last = _run(B, circuit, x)
    try:
        _assert_columns(B, circuit, x, cols, outs)
        # the device path ran: every cell of the plan was written by a kernel, in about one launch per layout op
        assert last["cells_written"] == plan.n_cells == dev.n_cells and last["failed"] == 0
        assert dev.n_records == plan.n_records and dev.n_ops == plan.n_ops
        assert plan.n_records <= last["launches"] <= 4 * plan.n_ops
        assert last["device_ms"] > 0
        # the same plan, other inputs, the same columns (dirty from the first run: they are zero-filled by the run)
        x2 = [(-v) % 7 - 3 for v in x]
        cols2, outs2 = dev.run(x2, columns=cols)
        assert cols2 is cols
        _assert_columns(B, circuit, x2, cols, outs2)
    finally:
        for c in cols:
            c.free()
        dev.free()


def test_out_of_range_input_is_reported_and_the_process_goes_on(hip):
    from ezkl_amd import backend as B, witness_plan as WP
    circuit, x = _relu_only(2)
    plan = WP.record_plan(circuit)
    dev = B.WitnessPlan(plan.to_bytes())
    cols = dev.alloc_columns()
    try:
        with pytest.raises(B.WitnessError, match="value exceeds the decomposition range.*decompose record") as e:
            dev.run([128 * 128, 0, 0], columns=cols)
        assert dev.last["failed"] >= 1 and dev.last["cells_written"] < plan.n_cells
        rec, elem = dev.last["first"]
        assert plan.records[rec, 0] == WP.HINT and "record %d, element %d" % (rec, elem) in str(e.value)
        with pytest.raises(AssertionError, match="record %d, element %d" % (rec, elem)):          # the host interpreter names the same cell
            WP.run_plan_host(plan, [128 * 128, 0, 0])
        with pytest.raises(B.WitnessError, match="decompose"):
            dev.run([0, -(1 << 40), 0], columns=cols)
        # the next valid run in the same process, into the same columns, is correct
        _, outs = dev.run(x, columns=cols)
        _assert_columns(B, circuit, x, cols, outs)
        assert dev.last["failed"] == 0 and dev.last["cells_written"] == plan.n_cells
        with pytest.raises(ValueError, match="inputs"):
            dev.run([1, 2], columns=cols)
    finally:
        for c in cols:
            c.free()
        dev.free()


def test_upload_refuses_a_bad_blob(hip):
    from ezkl_amd import backend as B
    from test_witness_plan_cpu import _bad_plans
    plan, bad = _bad_plans()
    for what, q in bad:
        with pytest.raises(ValueError, match=what):
            B.WitnessPlan(q.to_bytes())
    B.WitnessPlan(plan.to_bytes()).free()


def _keygen(circuit, x):
    from ezkl_amd import backend as B, ezkl_layout as EL, native as NV
    cs, fixed, copies, reg = circuit.keygen_inputs(x)
    bg, bgl = B.gen_srs(circuit.k, 0x5eed)
    pk = NV.NativeProvingKey(NV.NativeCircuit(cs), bg, EL.cols_to_mont(fixed, B), copies)
    pk.set_selectors(reg.selector_rows())
    return pk, bg, bgl, (cs, fixed, copies)


def test_create_proof_takes_device_columns_and_leaves_them_alone(hip):
    """all-numpy, all-DeviceBuffer and a mix give the same proof bytes; the caller's device columns are unchanged (the blinding rows go
    into the prover's copy)"""
    from ezkl_amd import backend as B, ezkl_layout as EL, native as NV
    circuit, x = CASES["mlp_k9_w2_3_blocks"]()
    adv, inst = circuit.witness(x)
    host = EL.cols_to_mont(adv)
    pk, bg, bgl, _ = _keygen(circuit, x)
    plan, dev, cols, outs, _ = _run(B, circuit, x)
    try:
        n = 1 << circuit.k
        before = [c.to_numpy(shape=(n, 4)).copy() for c in cols]
        ref = NV.create_proof(pk, bg, bgl, host, seed=7, instances=inst)
        assert NV.create_proof(pk, bg, bgl, list(cols), seed=7, instances=inst) == ref
        mixed = [c if i % 2 else h for i, (c, h) in enumerate(zip(cols, host))]
        assert NV.create_proof(pk, bg, bgl, mixed, seed=7, instances=inst) == ref
        signed = [[v if v < EL.R // 2 else v - EL.R for v in col] for col in adv]
        small = [all(abs(v) < 1 << 62 for v in col) for col in signed]             # (the inverses of equals_zero are not small)
        assert sum(small) >= 2
        mixed3 = [cols[i] if i % 3 == 0 else np.array(signed[i], np.int64) if small[i] else host[i] for i in range(len(cols))]
        assert NV.create_proof(pk, bg, bgl, mixed3, seed=7, instances=inst) == ref
        for c, b in zip(cols, before):
            assert c.to_numpy(shape=(n, 4)).tobytes() == b.tobytes(), "create_proof modified the caller's device column"
        with pytest.raises(ValueError, match="device column"):
            NV.create_proof(pk, bg, bgl, [B.DeviceView(cols[0].ptr, 32, cols[0])] + list(cols[1:]), seed=7, instances=inst)
        # a sharded constraint system (here: a world of one) refuses the format by name; back on one context it is taken again
        pk.circuit.set_shard(None, None)
        with pytest.raises(RuntimeError, match="device-resident advice columns are for the single-context prover"):
            NV.create_proof(pk, bg, bgl, mixed, seed=7, instances=inst)
        NV._check(NV.load().ezkl_prover_cs_set_shard(pk.circuit.h, 0, 0, None, None), "ezkl_prover_cs_set_shard")
        assert NV.create_proof(pk, bg, bgl, mixed, seed=7, instances=inst) == ref
    finally:
        for c in cols:
            c.free()
        dev.free(); bg.free(); bgl.free()


def test_execute_prove_device_and_host_write_the_same_proof(hip, tmp_path):
    """the k = 8 file chain of tests/test_execute.py: gen-srs -> gen-witness -> setup -> prove -> verify, with the witness made on the
    device and on the host under the same det-prove seed"""
    from ezkl_amd import backend as B, codecs, execute as X, witness_plan as WP
    ra = dict(json.load(open(os.path.join(FX.G, "settings_k6.json")))["run_args"], logrows=8)
    compiled = tmp_path / "model.compiled.json"
    compiled.write_text(json.dumps({"model": "mlp", "run_args": ra, "weights": [FIXTURE_W], "biases": [FIXTURE_B]}))
    srs, wit = tmp_path / "kzg8.srs", tmp_path / "witness.json"
    vk_path, pk_path = tmp_path / "vk.key", tmp_path / "pk.key"
    X.gen_srs(str(srs), 8, secret=0x5eed)
    X.gen_witness(str(compiled), {"input_data": [[1.5417295, 0.5346153, 1.2172532]]}, output=str(wit))
    X.setup(str(compiled), str(srs), str(vk_path), str(pk_path))
    circuit, _ = X._load_circuit(str(compiled))
    blob = open(str(pk_path) + ".wplan", "rb").read()
    assert blob == WP.record_plan(circuit).to_bytes() and WP.peek(blob)["param_hash"] == WP.params_hash(circuit)
    host = X.prove(str(wit), str(compiled), str(pk_path), str(tmp_path / "host.json"), str(srs), X.CheckMode.SAFE, seed=7, synthesis="host",
                   report=(how := {}))
    assert how == dict(path="host")
    devp = X.prove(str(wit), str(compiled), str(pk_path), str(tmp_path / "dev.json"), str(srs), X.CheckMode.SAFE, seed=7, synthesis="device",
                   report=how)
    assert how["path"] == "device" and how["cells_written"] == WP.peek(blob)["n_cells"]
    pj_dev, pj_host = [codecs.read_proof_json((tmp_path / f).read_text()) for f in ("dev.json", "host.json")]
    assert devp == host and pj_dev["proof"] == pj_host["proof"] == host and pj_dev["instances"] == pj_host["instances"]
    assert X.verify(str(tmp_path / "dev.json"), str(compiled), str(vk_path), str(srs))
    # "auto" below the GPU cutoff (k <= HIP_SMALL_K) is the host path, as before
    auto = X.prove(str(wit), str(compiled), str(pk_path), str(tmp_path / "auto.json"), str(srs), seed=7, report=how)
    assert auto == host and how == dict(path="host")
    # a plan file that belongs to another circuit is not used: a fresh one is recorded, the proof is the same
    other = dict(ra)
    compiled2 = tmp_path / "other.compiled.json"
    compiled2.write_text(json.dumps({"model": "mlp", "run_args": other, "weights": [[[1, 0, 0]] * 4], "biases": [[0, 0, 0, 0]]}))
    open(str(pk_path) + ".wplan", "wb").write(WP.record_plan(X._load_circuit(str(compiled2))[0]).to_bytes())
    assert X.prove(str(wit), str(compiled), str(pk_path), str(tmp_path / "dev2.json"), str(srs), seed=7, synthesis="device") == host
    os.remove(str(pk_path) + ".wplan")
    assert X.prove(str(wit), str(compiled), str(pk_path), str(tmp_path / "dev3.json"), str(srs), seed=7, synthesis="device") == host
    # the device's outputs are checked against the witness file's, as the host's are
    w = json.load(open(wit)); w["outputs"][0][0] = "01" + "00" * 31
    (tmp_path / "w.json").write_text(json.dumps(w))
    with pytest.raises(ValueError, match="outputs"):
        X.prove(str(tmp_path / "w.json"), str(compiled), str(pk_path), str(tmp_path / "p.json"), str(srs), synthesis="device")


def test_bench_mlp_k14_columns_and_mock(hip):
    """a size where the grids are not trivial: the bench MLP at k = 14 (tools/bench_circuits.py, base 128) -- columns equal, and the mock
    prover finds no failing gate, lookup or copy on the device-made columns"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_circuits as BC
    from ezkl_amd import backend as B, ezkl_layout as EL, native as NV
    circuit, x = BC.mlp_circuit(14, np.random.default_rng(1), base=128)
    plan, dev, cols, outs, last = _run(B, circuit, x)
    try:
        _assert_columns(B, circuit, x, cols, outs)
        assert last["cells_written"] == plan.n_cells and plan.n_records <= last["launches"] <= 4 * plan.n_ops
        assert last["launches"] < 400, "launches follow the layout ops of a layer, not its rows or dot steps"
        cs, fixed, copies, reg = circuit.keygen_inputs(x)
        n = 1 << circuit.k
        records, totals = NV.mock(cs, EL.cols_to_mont(fixed, B), copies, [c.to_numpy(shape=(n, 4)) for c in cols], instances=[outs])
        assert list(totals) == [0, 0, 0] and not records
    finally:
        for c in cols:
            c.free()
        dev.free()


def test_setup_and_prove_of_a_circuit_the_recorder_refuses(hip, tmp_path, monkeypatch):
    """a weight beyond int64: `setup` writes both keys and no plan, `prove` in its default mode takes the host path also where the GPU gate
    is open, and only synthesis="device" raises"""
    from ezkl_amd import execute as X, witness_plan as WP
    ra = dict(json.load(open(os.path.join(FX.G, "settings_k6.json")))["run_args"], logrows=8)
    compiled = tmp_path / "big.compiled.json"
    compiled.write_text(json.dumps({"model": "mlp", "run_args": ra, "weights": [[[1 << 70, 0, 0]] * 4], "biases": [[0, 0, 0, 0]]}))
    srs, wit = tmp_path / "kzg8.srs", tmp_path / "witness.json"
    vk_path, pk_path = tmp_path / "vk.key", tmp_path / "pk.key"
    X.gen_srs(str(srs), 8, secret=0x5eed)
    X.gen_witness(str(compiled), {"input_data": [[0.0, 0.0, 0.0]]}, output=str(wit))
    open(str(pk_path) + ".wplan", "wb").write(b"stale")            # a plan left by an earlier key at this path goes
    X.setup(str(compiled), str(srs), str(vk_path), str(pk_path))
    assert vk_path.exists() and pk_path.exists() and not os.path.exists(str(pk_path) + ".wplan")
    monkeypatch.setenv("ENABLE_HIP_GPU", "1")
    monkeypatch.setenv("HIP_SMALL_K", "4")
    X.prove(str(wit), str(compiled), str(pk_path), str(tmp_path / "p.json"), str(srs), X.CheckMode.SAFE, seed=7, report=(how := {}))
    assert how == dict(path="host") and X.verify(str(tmp_path / "p.json"), str(compiled), str(vk_path), str(srs))
    with pytest.raises(WP.PlanError, match="a parameter beyond int64"):
        X.prove(str(wit), str(compiled), str(pk_path), str(tmp_path / "q.json"), str(srs), seed=7, synthesis="device")
