"""`execute` on artefact FILES of the two-phase families -- batched MLPs and the attention head (tests/batch_mlp_cases.py): setup (keys
and a two-phase plan) -> gen_witness on the host and from phase 0 of the plan (equal bytes) -> mock -> prove with the witness made on
the host and on the device (equal bytes at one seed) -> verify; a wrong output, a flipped proof byte, and a Prover session that meets a
refused witness between good ones."""
import json
import os

import numpy as np
import pytest

import batch_mlp_cases as F

pytestmark = pytest.mark.gpu
SEEDS = (31, 32)
NAMES = list(F.BATCH_CASES) + ["attention"]


@pytest.fixture(autouse=True)
def open_gate(monkeypatch):
    monkeypatch.setenv("ENABLE_HIP_GPU", "1")
    monkeypatch.setenv("HIP_SMALL_K", "4")


@pytest.fixture(scope="module")
def srs_files(hip, tmp_path_factory):
    """one test SRS per k, made on first use"""
    from ezkl_amd import execute as X
    d, made = tmp_path_factory.mktemp("srs"), {}
    def srs(k):
        if k not in made:
            made[k] = str(d / ("kzg%d.srs" % k))
            X.gen_srs(made[k], k, secret=0x5eed + k)
        return made[k]
    return srs


def _inputs(name):
    """(make the circuit, two inputs it accepts, one it refuses)"""
    if name == "attention":
        x = F.attention().default_inputs()
        return F.attention, [x, np.random.default_rng(9).integers(-4, 5, len(x)).tolist()], [0, 300] + [0] * (len(x) - 2)    # scores below the exp table
    spec, xs = F.BATCH_CASES[name]
    return (lambda: F.batch(spec)), xs[:2], xs[0][:-1] + [F.BOUND]                                                            # one past the decomposition bound


@pytest.fixture(scope="module")
def cases(hip, srs_files, tmp_path_factory):
    """name -> the case's files, made on first use: description, keys (and the plan next to them), one witness file per input"""
    from ezkl_amd import execute as X
    made = {}
    def case(name):
        if name in made:
            return made[name]
        make, xs, refused = _inputs(name)
        d = tmp_path_factory.mktemp(name)
        circuit = make()
        compiled = F.write_description(X, circuit, d / "circuit.json")
        c = dict(dir=str(d), compiled=compiled, srs=srs_files(circuit.k), vk=str(d / "vk.key"), pk=str(d / "pk.key"), make=make, xs=xs, refused=refused, witnesses=[])
        X.setup(compiled, c["srs"], c["vk"], c["pk"])
        for i, x in enumerate(xs):
            c["witnesses"].append(str(d / ("w%d.json" % i)))
            X.gen_witness(compiled, F.data(x), output=c["witnesses"][-1])
        made[name] = c
        return c
    return case


def _edited(case, which, name, edit):
    w = json.load(open(case["witnesses"][which]))
    edit(w)
    path = os.path.join(case["dir"], name)
    json.dump(w, open(path, "w"))
    return path


@pytest.mark.parametrize("name", NAMES)
def test_files_end_to_end_host_and_device_write_the_same_bytes(cases, name):
    from ezkl_amd import codecs, execute as X, witness_plan as WP
    c = cases(name)
    d, x = c["dir"], c["xs"][0]
    head = WP.peek(open(c["pk"] + ".wplan", "rb").read())
    assert head["param_hash"] == WP.params_hash(c["make"]()), "setup writes this circuit's plan next to the key"
    assert WP.WitnessPlan.from_bytes(open(c["pk"] + ".wplan", "rb").read()).n_phases == 2
    host = open(c["witnesses"][0], "rb").read()
    for i, kw in enumerate((dict(synthesis="device", pk_path=c["pk"]), dict(synthesis="auto", pk_path=c["pk"]))):
        out = os.path.join(d, "dev%d.json" % i)
        X.gen_witness(c["compiled"], F.data(x), output=out, **kw)
        assert open(out, "rb").read() == host, "gen_witness %r differs from the host's file" % (kw,)
    with pytest.raises(ValueError):
        X.gen_witness(c["compiled"], F.data(c["refused"]), synthesis="device", pk_path=c["pk"])
    # mock
    assert X.mock(c["witnesses"][0], c["compiled"]) == ""
    lying = _edited(c, 0, "lying.json", lambda w: w["outputs"][0].__setitem__(0, codecs.felt_to_hex_le(12345)))
    with pytest.raises(X.MockError, match="copy") as e:
        X.mock(lying, c["compiled"])
    assert e.value.totals[0] == 0 and e.value.totals[2] >= 1, "a wrong output is a failing copy into the instance column, nothing else"
    # prove: host and device synthesis at one seed
    how, proofs = {}, {}
    for synthesis in ("host", "device"):
        path = os.path.join(d, "proof_%s.json" % synthesis)
        proofs[synthesis] = X.prove(c["witnesses"][0], c["compiled"], c["pk"], path, c["srs"], seed=SEEDS[0], synthesis=synthesis, report=how)
        assert how["path"] == synthesis
        assert X.verify(path, c["compiled"], c["vk"], c["srs"]) and X.verify(path, c["compiled"], c["pk"], c["srs"])
    assert proofs["host"] == proofs["device"]
    assert sorted(how["phase_ms"]) == [0, 1] and all(ms >= 0 for ms in how["phase_ms"].values())
    with pytest.raises(ValueError, match="outputs"):
        X.prove(lying, c["compiled"], c["pk"], os.path.join(d, "never.json"), c["srs"], seed=SEEDS[0], synthesis="device")
    # one flipped proof byte
    pj = codecs.read_proof_json(open(os.path.join(d, "proof_host.json")).read())
    bad = bytearray(pj["proof"])
    bad[len(bad) // 2] ^= 1
    flipped = os.path.join(d, "flipped.json")
    open(flipped, "w").write(codecs.write_proof_json(bytes(bad), pj["instances"]))
    assert not X.verify(flipped, c["compiled"], c["vk"], c["srs"])


@pytest.mark.parametrize("name", NAMES)
def test_a_session_meets_a_refused_witness_between_good_ones(cases, name):
    from ezkl_amd import backend as B, codecs, execute as X
    c = cases(name)
    refused = _edited(c, 1, "refused.json", lambda w: w["inputs"].__setitem__(0, [codecs.felt_to_hex_le(v % X.EL.R) for v in c["refused"]]))
    with pytest.raises(AssertionError):
        c["make"]().synthesize(c["refused"])
    with X.Prover(c["compiled"], c["pk"], c["srs"], synthesis="device") as p:
        assert p.plan is not None and p.plan.n_phases == 2 and len(p._cols) == p.plan.n_advice
        cols = [col.ptr for col in p._cols]
        how = {}
        first = p.prove(c["witnesses"][0], seed=SEEDS[0], report=how)
        assert how["path"] == "device" and sorted(how["phase_ms"]) == [0, 1] and all(ms >= 0 for ms in how["phase_ms"].values())
        assert "create_proof" in how["stages"]
        second = p.prove(c["witnesses"][1], os.path.join(c["dir"], "session1.json"), seed=SEEDS[1])
        assert second != first
        with pytest.raises(B.WitnessError):
            p.prove(refused, seed=SEEDS[1])
        assert p.prove(c["witnesses"][0], seed=SEEDS[0]) == first, "the proof after a refused witness differs from the first, at its seed"
        assert [col.ptr for col in p._cols] == cols, "one set of resident columns"
    assert X.verify(os.path.join(c["dir"], "session1.json"), c["compiled"], c["vk"], c["srs"])
    with X.Prover(c["compiled"], c["pk"], c["srs"], synthesis="host") as p:    # the same callable over the host layout
        how = {}
        assert p.plan is None and p.prove(c["witnesses"][0], seed=SEEDS[0], report=how) == first and how == dict(how, path="host")
        with pytest.raises(AssertionError):
            p.prove(refused, seed=SEEDS[1])
        assert p.prove(c["witnesses"][1], seed=SEEDS[1]) == second
