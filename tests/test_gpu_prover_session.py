"""execute.Prover: one load, many proofs.  The circuit, its constraint system (from the key's selector rows), the proving key, both base
sets and the witness plan with its advice columns are loaded once; every proof of the session equals `execute.prove`'s byte for byte
(det-prove seed), whichever way the witness is made, and a refused witness costs the session nothing.  Run on the reference's own k = 6
files (its key re-committed under the test SRS) and on the k = 8 `1l_relu` description of tests/test_execute.py, with the GPU gate open."""
import gc
import json
import os

import pytest

import fixture_k6 as FX

pytestmark = pytest.mark.gpu
SEEDS = (11, 12, 13)


@pytest.fixture(autouse=True)
def open_gate(monkeypatch):
    monkeypatch.setenv("ENABLE_HIP_GPU", "1")
    monkeypatch.setenv("HIP_SMALL_K", "4")


def _reference_proofs(X, case):
    """execute.prove(synthesis="host") of every witness at its seed: what each session proof must equal"""
    out = []
    for i, (wit, seed) in enumerate(zip(case["witnesses"], SEEDS)):
        path = os.path.join(case["dir"], "ref%d.json" % i)
        out.append(X.prove(wit, case["compiled"], case["pk"], path, case["srs"], seed=seed, recommit=case["recommit"], synthesis="host"))
    return out


@pytest.fixture(scope="module")
def golden_k6(hip, tmp_path_factory):
    from ezkl_amd import execute as X
    d = tmp_path_factory.mktemp("golden_k6")
    g = lambda name: os.path.join(FX.G, name)
    wits = [g("witness_k6.json")]
    for i, x in enumerate(([-3.0, -100.0, 77.0], [5.0, 0.0, -7.0])):
        wits.append(str(d / ("w%d.json" % i)))
        X.gen_witness(g("model_k6.compiled"), {"input_data": [x]}, output=wits[-1])
    case = dict(dir=str(d), compiled=g("model_k6.compiled"), pk=g("pk_k6.key"), srs=g("kzg_k6.srs"), recommit=True, witnesses=wits)
    case["proofs"] = _reference_proofs(X, case)
    return case


@pytest.fixture(scope="module")
def relu_k8(hip, tmp_path_factory):
    from ezkl_amd import execute as X
    d = tmp_path_factory.mktemp("relu_k8")
    ra = dict(logrows=8, num_inner_cols=2, decomp_base=128, decomp_legs=2, input_scale=7)
    compiled = d / "1l_relu.compiled.json"
    compiled.write_text(json.dumps({"model": "mlp", "run_args": ra, "weights": [], "biases": [], "n_inputs": 3, "relu_first": True}))
    X.gen_srs(str(d / "kzg8.srs"), 8, secret=0x5eed)
    wits = []
    for i, x in enumerate(([-0.40077725052833557, 2.493845224380493, 0.5796360969543457], [1.0, -2.0, 3.0], [0.0, 100.0, -100.0])):
        wits.append(str(d / ("w%d.json" % i)))
        X.gen_witness(str(compiled), {"input_data": [x]}, output=wits[-1])
    X.setup(str(compiled), str(d / "kzg8.srs"), str(d / "vk.key"), str(d / "pk.key"))
    assert os.path.exists(str(d / "pk.key") + ".wplan")
    case = dict(dir=str(d), compiled=str(compiled), pk=str(d / "pk.key"), vk=str(d / "vk.key"), srs=str(d / "kzg8.srs"), recommit=False, witnesses=wits)
    case["proofs"] = _reference_proofs(X, case)
    return case


def _open(X, case, synthesis):
    return X.Prover(case["compiled"], case["pk"], case["srs"], recommit=case["recommit"], synthesis=synthesis)


@pytest.mark.parametrize("synthesis", ["device", "host"])
@pytest.mark.parametrize("which", ["golden_k6", "relu_k8"])
def test_three_witnesses_in_one_session_equal_execute_prove(which, synthesis, request):
    from ezkl_amd import codecs, execute as X
    case = request.getfixturevalue(which)
    assert len(set(case["proofs"])) == 3
    with _open(X, case, synthesis) as p:
        assert set(p.opened) >= {"circuit", "constraint_system", "srs_read", "srs_to_device", "key", "plan"}
        for i, (wit, seed, want) in enumerate(zip(case["witnesses"], SEEDS, case["proofs"])):
            path = os.path.join(case["dir"], "%s_%d.json" % (synthesis, i))
            how = {}
            assert p.prove(wit, path, seed=seed, report=how) == want, "proof %d differs from execute.prove's" % i
            assert how["path"] == synthesis and {"witness_read", "synthesis", "create_proof", "proof_write"} <= set(how["stages"])
            assert ("cells_written" in how) == (synthesis == "device") and how["create_proof_breakdown"]["total"] > 0
            assert codecs.read_proof_json(open(path).read())["proof"] == want
            if case["recommit"]:
                assert X.verify(path, case["compiled"], case["pk"], case["srs"], recommit=True)
            else:
                assert X.verify(path, case["compiled"], case["vk"], case["srs"])
        assert p.prove(case["witnesses"][0], seed=SEEDS[0], check_mode=X.CheckMode.SAFE) == case["proofs"][0]        # no file asked for, none written


def test_proving_lays_nothing_out_once_the_keys_exist(relu_k8, monkeypatch):
    from ezkl_amd import execute as X, ezkl_layout as EL
    def no_layout(self, *a, **kw):
        raise AssertionError("the prover laid the circuit out")
    monkeypatch.setattr(EL.MlpCircuit, "synthesize", no_layout)
    case = relu_k8
    with _open(X, case, "device") as p:
        assert p.prove(case["witnesses"][1], seed=SEEDS[1]) == case["proofs"][1]
    out = os.path.join(case["dir"], "nolayout.json")
    assert X.prove(case["witnesses"][2], case["compiled"], case["pk"], out, case["srs"], seed=SEEDS[2], synthesis="device") == case["proofs"][2]
    assert X.verify(out, case["compiled"], case["vk"], case["srs"])


def test_a_session_loads_once_and_holds_its_memory(relu_k8, monkeypatch):
    from ezkl_amd import backend as B, execute as X, native as NV
    calls = dict(plan=0, key=0)
    plan_init, from_file = B.WitnessPlan.__init__, NV.NativeProvingKey.from_file.__func__
    def counted_plan(self, blob):
        calls["plan"] += 1
        plan_init(self, blob)
    def counted_key(cls, *a, **kw):
        calls["key"] += 1
        return from_file(cls, *a, **kw)
    monkeypatch.setattr(B.WitnessPlan, "__init__", counted_plan)
    monkeypatch.setattr(NV.NativeProvingKey, "from_file", classmethod(counted_key))
    case, stats = relu_k8, []
    with _open(X, case, "device") as p:
        for i in range(4):
            assert p.prove(case["witnesses"][i % 3], seed=SEEDS[i % 3]) == case["proofs"][i % 3]
            stats.append(B.pool_stats())
    assert calls == dict(plan=1, key=1)
    assert stats[1] == stats[3], "the session's footprint moved between proof 2 and proof 4"


def _edited(case, name, edit):
    w = json.load(open(case["witnesses"][0]))
    edit(w)
    path = os.path.join(case["dir"], name)
    json.dump(w, open(path, "w"))
    return path


def test_a_refused_witness_leaves_the_session_usable(relu_k8):
    from ezkl_amd import backend as B, codecs, execute as X
    case = relu_k8
    def too_large(w): w["inputs"][0][0] = codecs.felt_to_hex_le(128 * 128)             # base^legs: the first value the decomposition cannot hold
    def wrong_output(w): w["outputs"][0][0] = "01" + "00" * 31
    beyond, lying = _edited(case, "beyond.json", too_large), _edited(case, "lying.json", wrong_output)
    with _open(X, case, "device") as p:                                                # a fresh session: the bytes to compare with, and a warm library
        fresh = p.prove(case["witnesses"][1], seed=SEEDS[1])
    assert fresh == case["proofs"][1]
    gc.collect()                                                                       # nothing of an earlier test left to free in between
    B.pool_trim()
    before = B.pool_stats()
    p = _open(X, case, "device")
    try:
        p.prove(case["witnesses"][0], seed=SEEDS[0])
        held = B.pool_stats()["live"]
        with pytest.raises(B.WitnessError, match="value exceeds the decomposition range.*decompose record"):
            p.prove(beyond, seed=SEEDS[0])
        assert B.pool_stats()["live"] == held
        with pytest.raises(ValueError, match="outputs"):
            p.prove(lying, seed=SEEDS[0], report=(how := {}))
        assert how["path"] == "device" and B.pool_stats()["live"] == held
        assert p.prove(case["witnesses"][1], seed=SEEDS[1]) == fresh
    finally:
        p.close()
    B.pool_trim()
    assert B.pool_stats() == before, "the session did not give back what it took"


def test_closed_session_raises_and_the_report_keeps_its_keys(relu_k8):
    from ezkl_amd import execute as X
    case = relu_k8
    p = _open(X, case, "device")
    p.prove(case["witnesses"][0], seed=SEEDS[0])
    p.close()
    p.close()                                                                           # closing twice is harmless
    with pytest.raises(RuntimeError, match="closed"):
        p.prove(case["witnesses"][0], seed=SEEDS[0])
    out = os.path.join(case["dir"], "report.json")
    X.prove(case["witnesses"][0], case["compiled"], case["pk"], out, case["srs"], seed=SEEDS[0], synthesis="host", report=(how := {}))
    assert set(how) >= {"path"} and how["path"] == "host"
    X.prove(case["witnesses"][0], case["compiled"], case["pk"], out, case["srs"], seed=SEEDS[0], synthesis="device", report=how)
    assert set(how) >= {"path", "failed", "first", "cells_written", "launches", "device_ms"} and how["path"] == "device"
    with pytest.raises(ValueError, match="synthesis must be"):
        X.Prover(case["compiled"], case["pk"], case["srs"], synthesis="gpu")
