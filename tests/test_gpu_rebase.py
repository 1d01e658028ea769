"""The rebase division on the device: the DIVC branch of the element-wise witness kernel (csrc/witness.hip) against the host interpreter on
hand-built plans at the block edges, the recorded plans of tests/test_rebase_cpu.py against the layout engine, a dividend beyond the
exact-division range reported by (record, element) without ending the process, proofs from device columns equal to proofs from host
columns, and the file chain gen-srs -> gen-witness -> setup -> prove -> verify, a Prover session and `mock` on a description at ezkl's
default scales."""
import json
import os

import pytest

from test_gpu_witness import _assert_columns, _keygen
from test_rebase_cpu import CASES, description, div_plan

pytestmark = pytest.mark.gpu
K = 9
EDGE = (1 << 52) - 1


def _dividends(count, d, shift):
    """zero, both signs, the values at and next to a half (for an even d the half is exact), and the ends of the exact range"""
    h = d // 2
    vals = [0, 1, -1, h, -h, h + 1, -(h + 1), max(h - 1, 0), 3 * d + h, -(3 * d + h), EDGE, -EDGE, 5 * d, -(5 * d) - h, 12345, -99999, 3 * d + h + 1, EDGE - 1]
    return [vals[(i + shift) % len(vals)] for i in range(count)]


@pytest.mark.parametrize("d", [2, 3, 128, 2 ** 32 - 1])
@pytest.mark.parametrize("count", [1, 255, 256, 257])
def test_hand_built_plans_equal_the_host_interpreter(hip, count, d):
    from ezkl_amd import backend as B, ezkl_layout as EL, witness_plan as WP
    plan = div_plan(count, d, K)
    dev = B.WitnessPlan(plan.to_bytes())
    cols = dev.alloc_columns()
    try:
        for shift in (0, 3, 10):                                  # (one lane: 0, a half, the largest dividend)
            x = _dividends(count, d, shift)
            ref_cols, ref_outs = WP.run_plan_host(plan, x)
            _, outs = dev.run(x, columns=cols)
            assert outs == ref_outs
            assert dev.last["cells_written"] == plan.n_cells == 2 * count and dev.last["failed"] == 0
            for c, (got, ref) in enumerate(zip(cols, EL.cols_to_mont(ref_cols))):
                assert got.to_numpy(shape=(1 << K, 4)).tobytes() == ref.tobytes(), "column %d differs (count %d, d %d, shift %d)" % (c, count, d, shift)
    finally:
        for c in cols:
            c.free()
        dev.free()


@pytest.mark.parametrize("name", list(CASES))
def test_recorded_plans_equal_the_layout_engine(hip, name):
    from ezkl_amd import backend as B, witness_plan as WP
    circuit, xs = CASES[name]()
    plan = WP.record_plan(circuit)
    dev = B.WitnessPlan(plan.to_bytes())
    cols = dev.alloc_columns()
    try:
        for x in xs:                                              # every later input goes into the columns the one before left dirty
            _, outs = dev.run(x, columns=cols)
            _assert_columns(B, circuit, x, cols, outs)
            assert dev.last["cells_written"] == plan.n_cells and dev.last["failed"] == 0
            assert plan.n_records <= dev.last["launches"] <= 4 * plan.n_ops
    finally:
        for c in cols:
            c.free()
        dev.free()


def test_a_dividend_beyond_the_exact_range_is_reported_and_the_process_goes_on(hip):
    from ezkl_amd import backend as B, ezkl_layout as EL, witness_plan as WP
    count, d = 300, 3
    plan = div_plan(count, d, K)
    dev = B.WitnessPlan(plan.to_bytes())
    cols = dev.alloc_columns()
    try:
        good = _dividends(count, d, 0)
        bad = list(good)
        bad[258], bad[290] = 1 << 52, -(1 << 52)
        with pytest.raises(AssertionError, match=r"rebase dividend outside the exact-division range \(div record 1, element 258"):
            WP.run_plan_host(plan, bad)
        with pytest.raises(B.WitnessError, match=r"rebase dividend outside the exact-division range \(div record 1, element 258"):
            dev.run(bad, columns=cols)
        assert dev.last["failed"] == 2 and dev.last["first"] == (1, 258) and dev.last["cells_written"] == plan.n_cells - 2
        quotients = cols[1].to_numpy(shape=(1 << K, 4))
        assert not quotients[258].any() and not quotients[290].any(), "a refused lane wrote its cell"
        ok = [i for i in range(count) if i not in (258, 290)]
        want = EL.cols_to_mont([[EL.round_div(good[i], d) % EL.R for i in ok]])[0]
        assert quotients[ok].tobytes() == want.tobytes()
        # the next valid run in the same process, into the same columns
        ref_cols, ref_outs = WP.run_plan_host(plan, good)
        _, outs = dev.run(good, columns=cols)
        assert outs == ref_outs and dev.last["failed"] == 0 and dev.last["cells_written"] == plan.n_cells
        for got, ref in zip(cols, EL.cols_to_mont(ref_cols)):
            assert got.to_numpy(shape=(1 << K, 4)).tobytes() == ref.tobytes()
    finally:
        for c in cols:
            c.free()
        dev.free()


def test_proofs_from_device_columns_equal_proofs_from_host_columns(hip, tmp_path):
    from ezkl_amd import backend as B, codecs, execute as X, ezkl_layout as EL, native as NV, witness_plan as WP
    circuit, xs = CASES["two_layer_relu_last_d128"]()
    x = xs[0]
    adv, inst = circuit.witness(x)
    pk, bg, bgl, (cs, fixed, copies) = _keygen(circuit, x)
    X.gen_srs(str(tmp_path / "kzg.srs"), circuit.k, secret=0x5eed)          # the secret of _keygen's bases: g2 / s_g2 for the SAFE check
    g2, s_g2 = codecs.read_srs_g2(str(tmp_path / "kzg.srs"))
    dev = B.WitnessPlan(WP.record_plan(circuit).to_bytes())
    cols, outs = dev.run(x)
    try:
        assert [outs] == inst
        ref = NV.create_proof(pk, bg, bgl, EL.cols_to_mont(adv), seed=7, instances=inst, check_mode="SAFE", g2=g2, s_g2=s_g2)
        assert NV.create_proof(pk, bg, bgl, list(cols), seed=7, instances=inst, check_mode="SAFE", g2=g2, s_g2=s_g2) == ref
        n = 1 << circuit.k
        records, totals = NV.mock(cs, EL.cols_to_mont(fixed, B), copies, [c.to_numpy(shape=(n, 4)) for c in cols], instances=[outs])
        assert list(totals) == [0, 0, 0] and not records
    finally:
        for c in cols:
            c.free()
        dev.free(); bg.free(); bgl.free()


def test_the_file_chain_a_session_and_mock_at_the_default_scales(hip, tmp_path, monkeypatch):
    from ezkl_amd import codecs, execute as X, witness_plan as WP
    monkeypatch.setenv("ENABLE_HIP_GPU", "1")                     # the gate open, as tests/test_gpu_prover_session.py opens it
    monkeypatch.setenv("HIP_SMALL_K", "4")
    compiled, _, _ = description(tmp_path, logrows=K)
    srs, vk, pk = (str(tmp_path / f) for f in ("kzg9.srs", "vk.key", "pk.key"))
    wits = [str(tmp_path / ("w%d.json" % i)) for i in range(2)]
    X.gen_srs(srs, K, secret=0x5eed)
    outs = [X.gen_witness(compiled, {"input_data": [x]}, output=w)["outputs"] for x, w in zip(([0.7734375, -1.0, 0.6015625], [-0.9921875, -0.9921875, -0.9921875]), wits)]
    assert outs[0] != outs[1]
    X.setup(compiled, srs, vk, pk)
    circuit, _ = X._load_circuit(compiled)
    blob = open(pk + ".wplan", "rb").read()
    assert blob == WP.record_plan(circuit).to_bytes() and WP.DIVC in WP.WitnessPlan.from_bytes(blob).records[:, 0].tolist()
    how = {}
    devp = X.prove(wits[0], compiled, pk, str(tmp_path / "dev.json"), srs, X.CheckMode.SAFE, seed=7, synthesis="device", report=how)
    assert how["path"] == "device" and how["cells_written"] == WP.peek(blob)["n_cells"]
    assert X.verify(str(tmp_path / "dev.json"), compiled, vk, srs)
    assert X.prove(wits[0], compiled, pk, str(tmp_path / "host.json"), srs, X.CheckMode.SAFE, seed=7, synthesis="host", report=how) == devp
    assert how == dict(path="host")
    with X.Prover(compiled, pk, srs, synthesis="device") as p:
        proofs = []
        for i, w in enumerate(wits):
            proofs.append(p.prove(w, str(tmp_path / ("s%d.json" % i)), check_mode=X.CheckMode.SAFE, seed=7, report=how))
            assert how["path"] == "device" and X.verify(str(tmp_path / ("s%d.json" % i)), compiled, vk, srs)
    assert proofs[0] == devp and proofs[0] != proofs[1]
    swapped = str(tmp_path / "swapped.json")                      # the first proof with the second witness's public outputs
    inst1 = codecs.read_proof_json(open(str(tmp_path / "s1.json")).read())["instances"]
    open(swapped, "w").write(codecs.write_proof_json(proofs[0], inst1))
    assert not X.verify(swapped, compiled, vk, srs)
    assert X.mock(wits[0], compiled) == ""
    w = json.load(open(wits[0])); w["outputs"][0][0] = "01" + "00" * 31
    lying = str(tmp_path / "lying.json")
    open(lying, "w").write(json.dumps(w))
    with pytest.raises(X.MockError):
        X.mock(lying, compiled)
    assert os.path.exists(vk)
