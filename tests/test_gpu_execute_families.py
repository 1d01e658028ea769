"""`execute` on artefact FILES of the conv, norm and pooled-classifier families (tests/execute_family_cases.py): setup -> gen_witness on the
host and from the plan (equal bytes) -> mock -> prove with the witness made on the host and on the device (equal bytes at one seed, and
equal to native.create_proof on circuit.witness) -> verify; a flipped proof byte, a wrong output, a witness the circuit refuses in the
middle of a Prover session, and the key of another description of the same family."""
import json
import os

import pytest

import execute_family_cases as F

pytestmark = pytest.mark.gpu
SEEDS = (21, 22, 23)
NAMES = list(F.CASES)


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


@pytest.fixture(scope="module")
def cases(hip, srs_files, tmp_path_factory):
    """name -> the family's files, made on first use: description, keys (and the plan next to them), one witness file per input"""
    from ezkl_amd import execute as X
    made = {}
    def case(name):
        if name in made:
            return made[name]
        make, xs, refused = F.CASES[name]
        d = tmp_path_factory.mktemp(name)
        circuit = make()
        compiled = F.write_description(X, circuit, d / "circuit.json")
        c = dict(dir=str(d), compiled=compiled, srs=srs_files(circuit.k), vk=str(d / "vk.key"), pk=str(d / "pk.key"), make=make, xs=xs, refused=refused, witnesses=[])
        X.setup(compiled, c["srs"], c["vk"], c["pk"])
        assert os.path.exists(c["pk"] + ".wplan"), "setup writes the witness plan next to the key"
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


def _refused_input(case):
    """an input the circuit's layout refuses: the case's own (past its lookup table), else the first of a few large ones that the host
    layout asserts on (past a decomposition or the exact-division range)"""
    if case["refused"] is not None:
        return case["refused"]
    n = len(case["xs"][0])
    for x in ([10 ** 7] * n, [10 ** 7 * (i % 3 + 1) for i in range(n)], [(-1) ** i * 10 ** 9 for i in range(n)]):
        try:
            case["make"]().synthesize(x)
        except AssertionError:
            return x
    raise AssertionError("no refused input found")


@pytest.mark.parametrize("name", NAMES)
def test_files_end_to_end_host_and_device_write_the_same_bytes(cases, name):
    from ezkl_amd import backend as B, codecs, execute as X, ezkl_layout as EL, native as NV
    c = cases(name)
    d, x = c["dir"], c["xs"][0]
    # gen_witness: the host's file, the device's from the plan next to the key, the device's from a fresh recording, "auto" with the gate open
    host = open(c["witnesses"][0], "rb").read()
    for i, kw in enumerate((dict(synthesis="device", pk_path=c["pk"]), dict(synthesis="device"), dict(synthesis="auto", pk_path=c["pk"]))):
        out = os.path.join(d, "dev%d.json" % i)
        X.gen_witness(c["compiled"], F.data(x), output=out, **kw)
        assert open(out, "rb").read() == host, "gen_witness %r differs from the host's file" % (kw,)
    w = json.loads(host)
    assert (w["min_lookup_inputs"], w["max_lookup_inputs"]) == F.expected_stats(name, c["make"](), x)
    # mock
    assert X.mock(c["witnesses"][0], c["compiled"]) == ""
    lying = _edited(c, 0, "lying.json", lambda w: w["outputs"][0].__setitem__(0, codecs.felt_to_hex_le(12345)))
    with pytest.raises(X.MockError, match="copy") as e:
        X.mock(lying, c["compiled"])
    assert e.value.totals[0] == 0 and e.value.totals[2] >= 1, "a wrong output is a failing copy into the instance column, nothing else"
    # prove: host and device synthesis, and the class path, at one seed
    how = {}
    proofs = {}
    for synthesis in ("host", "device"):
        path = os.path.join(d, "proof_%s.json" % synthesis)
        proofs[synthesis] = X.prove(c["witnesses"][0], c["compiled"], c["pk"], path, c["srs"], seed=SEEDS[0], synthesis=synthesis, report=how)
        assert how["path"] == synthesis
        assert X.verify(path, c["compiled"], c["vk"], c["srs"]) and X.verify(path, c["compiled"], c["pk"], c["srs"])
    assert proofs["host"] == proofs["device"]
    circuit = c["make"]()
    adv, inst = circuit.witness(x)
    with X.Prover(c["compiled"], c["pk"], c["srs"], synthesis="host") as p:      # the key and the bases as files load them; the witness as the class makes it
        direct = NV.create_proof(p.pk, p.bg, p.bgl, EL.cols_to_mont(adv, B), seed=SEEDS[0], instances=inst, g2=p.g2, s_g2=p.s_g2)
    assert direct == proofs["host"], "the file level and native.create_proof on circuit.witness differ"
    # one flipped proof byte
    pj = codecs.read_proof_json(open(os.path.join(d, "proof_host.json")).read())
    bad = bytearray(pj["proof"])
    bad[len(bad) // 2] ^= 1
    flipped = os.path.join(d, "flipped.json")
    open(flipped, "w").write(codecs.write_proof_json(bytes(bad), pj["instances"]))
    assert not X.verify(flipped, c["compiled"], c["vk"], c["srs"])
    with pytest.raises(ValueError, match="outputs"):
        X.prove(lying, c["compiled"], c["pk"], os.path.join(d, "never.json"), c["srs"], seed=SEEDS[0], synthesis="device")


@pytest.mark.parametrize("name", NAMES)
def test_a_session_of_three_witnesses_with_a_refused_one_in_between(cases, name):
    from ezkl_amd import backend as B, codecs, execute as X
    c = cases(name)
    alone = [X.prove(w, c["compiled"], c["pk"], os.path.join(c["dir"], "alone%d.json" % i), c["srs"], seed=s, synthesis="host")
             for i, (w, s) in enumerate(zip(c["witnesses"], SEEDS))]
    assert len(set(alone)) == 3
    x_bad = _refused_input(c)
    refused = _edited(c, 1, "refused.json", lambda w: w["inputs"].__setitem__(0, [codecs.felt_to_hex_le(v % X.EL.R) for v in x_bad]))
    with pytest.raises(ValueError):
        X.gen_witness(c["compiled"], F.data(x_bad), synthesis="device", pk_path=c["pk"])
    for synthesis in ("device", "host", "auto"):
        with X.Prover(c["compiled"], c["pk"], c["srs"], synthesis=synthesis) as p:
            assert (p.plan is not None) == (synthesis != "host") and len(p._cols) == (p.plan.n_advice if p.plan else 0)
            cols = [col.ptr for col in p._cols]
            how = {}
            assert p.prove(c["witnesses"][0], seed=SEEDS[0], report=how) == alone[0]
            assert how["path"] == ("host" if synthesis == "host" else "device")
            with pytest.raises(B.WitnessError if synthesis != "host" else AssertionError):
                p.prove(refused, seed=SEEDS[1])
            assert p.prove(c["witnesses"][1], seed=SEEDS[1]) == alone[1], "the proof after a refused witness differs from its stand-alone bytes"
            assert p.prove(c["witnesses"][2], os.path.join(c["dir"], "session2.json"), seed=SEEDS[2]) == alone[2]
            assert [col.ptr for col in p._cols] == cols, "one set of resident columns"
        assert X.verify(os.path.join(c["dir"], "session2.json"), c["compiled"], c["vk"], c["srs"])


@pytest.mark.parametrize("name", NAMES)
def test_the_key_of_another_description_of_the_family_does_not_serve(cases, srs_files, tmp_path, name):
    """the same shape with one other field that the key carries -- the conv's divisor (its lookup table), the classifier's decomposition base
    (its range table), the norm's eps (the zero_inverse constant); the private parameters are witness values, no key knows them -- : its
    key either does not belong or does not verify"""
    from ezkl_amd import execute as X
    c = cases(name)
    j = X.describe(c["make"]())
    if j["model"] == "conv":
        j["denom"] *= 2
    elif j["model"] == "pool_classifier":
        j["run_args"]["decomp_base"] //= 2
    else:
        j["eps"] *= 2
    compiled = str(tmp_path / "other.json")
    open(compiled, "w").write(json.dumps(j))
    vk, pk = str(tmp_path / "vk.key"), str(tmp_path / "pk.key")
    X.setup(compiled, c["srs"], vk, pk)
    proof = os.path.join(c["dir"], "for_other.json")
    X.prove(c["witnesses"][0], c["compiled"], c["pk"], proof, c["srs"], seed=SEEDS[0], synthesis="device")
    assert X.verify(proof, c["compiled"], c["vk"], c["srs"])
    for key, description in ((vk, c["compiled"]), (vk, compiled)):               # (the proof's own key decides, whichever description gives the shape)
        try:
            assert not X.verify(proof, description, key, c["srs"])
        except ValueError as e:
            assert "does not belong to this circuit" in str(e)
