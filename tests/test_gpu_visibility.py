"""Visibility on files, on the GPU: public inputs, Fixed and KZG-committed tensors of the MLP family through setup -> gen_witness -> prove
-> verify on artefact FILES, host and device synthesis byte for byte; the tie between a witness file's commitments and the first points of
a proof (`swap_proof_commitments`); the device-side commitment of a resident module column against PolyCommitChip::commit on the host
message at the lengths where the column count changes; and a Prover session on committed parameters.

No reference artefact with these visibilities exists offline: the yardsticks are the oracle's verifier (oracle/verifier.py), the mock
prover and the reference's code (src/graph/mod.rs:1945-2200, src/circuit/modules/polycommit.rs, src/pfsys/mod.rs:492-554)."""
import json
import os
import shutil

import numpy as np
import pytest

import fixture_k6 as FX
import visibility_cases as VC

pytestmark = pytest.mark.gpu

E2E = [("Public", "Fixed", "Public"), ("KZGCommit", "KZGCommit", "KZGCommit"), ("Public", "KZGCommit", "Public"), ("Private", "Fixed", "KZGCommit")]
SEED = 7
DATA, OTHER_DATA = {"input_data": [[3.0, -2.0, 7.0]]}, {"input_data": [[-4.0, 6.0, 1.0]]}
SRS_K6 = os.path.join(FX.G, "kzg_k6.srs")
_made = {}


@pytest.fixture(scope="module")
def root(hip, tmp_path_factory):
    return tmp_path_factory.mktemp("visibility")


def _chain(root, name, desc, srs, data=DATA):
    """setup -> gen_witness (host, device) -> prove (host, device) on files, once per name"""
    from ezkl_amd import execute as X
    if name in _made:
        return _made[name]
    d = root / name
    d.mkdir()
    p = lambda f: str(d / f)
    open(p("model.json"), "w").write(json.dumps(desc))
    info = X.setup(p("model.json"), srs, p("vk.key"), p("pk.key"))
    assert os.path.exists(p("pk.key") + ".wplan")
    wh = X.gen_witness(p("model.json"), data, output=p("w_host.json"), vk_path=p("vk.key"), srs_path=srs, synthesis="host")
    wd = X.gen_witness(p("model.json"), data, output=p("w_dev.json"), vk_path=p("vk.key"), srs_path=srs, synthesis="device", pk_path=p("pk.key"))
    how = {}
    proof_h = X.prove(p("w_host.json"), p("model.json"), p("pk.key"), p("proof_host.json"), srs, seed=SEED, synthesis="host")
    proof_d = X.prove(p("w_host.json"), p("model.json"), p("pk.key"), p("proof_dev.json"), srs, seed=SEED, synthesis="device", report=how)
    _made[name] = dict(dir=d, p=p, info=info, wh=wh, wd=wd, proof_h=proof_h, proof_d=proof_d, how=how, srs=srs, desc=desc)
    return _made[name]


def _oracle_accepts(case):
    """oracle/verifier.py on the key file's commitments and the proof file"""
    from oracle import pairing as E, pyref as pr, verifier as V
    from ezkl_amd import codecs, execute as X, plonk as P
    circuit, _ = X._load_circuit(case["p"]("model.json"))
    cs, raw = X._key_system(circuit, case["p"]("vk.key"))
    key = codecs.read_vk(raw, len(cs.perm), cs.n_selectors)
    vk = P.VerifyingKey()
    vk.cs = cs
    vk.fixed_commitments = [P.point_to_ints(pt) for pt in key["fixed_commitments"]]
    vk.sigma_commitments = [P.point_to_ints(pt) for pt in key["permutation_commitments"]]
    vk.digest = P.vk_digest(vk)
    srs = pr.parse_srs(open(case["srs"], "rb").read())
    pj = codecs.read_proof_json(open(case["p"]("proof_host.json")).read())
    return V.verify(vk, pr.g1_from_bytes(srs["g"][0]), E.g2_from_bytes(srs["g2"]), E.g2_from_bytes(srs["s_g2"]), pj["proof"], instances=pj["instances"])


def _leading_points(proof, count):
    from ezkl_amd import codecs
    return codecs.split_evm_proof(proof, count, 0)[0]


@pytest.mark.parametrize("tri", E2E, ids=VC.ids)
def test_end_to_end_on_files_host_and_device_agree(root, tri):
    from ezkl_amd import codecs, execute as X, ezkl_layout as EL
    case = _chain(root, VC.ids(tri), VC.description(tri), SRS_K6)
    p = case["p"]
    assert open(p("w_host.json"), "rb").read() == open(p("w_dev.json"), "rb").read()
    assert case["proof_h"] == case["proof_d"] and case["how"]["path"] == "device"
    n_committed = sum(v == "KZGCommit" for v in tri)
    assert case["info"]["n_advice"] == 18 + n_committed                       # the fixture shape's 18 model columns behind the modules'
    for key, v in zip(("processed_inputs", "processed_params", "processed_outputs"), tri):
        assert (case["wh"][key] is not None) == (v == "KZGCommit")
        if v == "KZGCommit":
            assert len(case["wh"][key]["polycommit"]) == 1 and len(case["wh"][key]["polycommit"][0]) == 1
    x = [3, -2, 7]
    outs = [int.from_bytes(bytes.fromhex(h), "little") for h in case["wh"]["outputs"][0]]
    want = ([v % EL.R for v in x] if tri[0] == "Public" else []) + (outs if tri[2] == "Public" else [])
    pj = codecs.read_proof_json(open(p("proof_host.json")).read())
    assert pj["instances"] == [want]
    assert X.verify(p("proof_host.json"), p("model.json"), p("vk.key"), case["srs"])
    assert X.verify(p("proof_dev.json"), p("model.json"), p("pk.key"), case["srs"])
    assert _oracle_accepts(case)
    assert X.mock(p("w_host.json"), p("model.json")) == ""
    if want:                                                                  # another public value: refused
        j = json.loads(open(p("proof_host.json")).read())
        j["instances"][0][0] = codecs.felt_to_hex_le((want[0] + 1) % EL.R)
        open(p("bad_instance.json"), "w").write(json.dumps(j))
        assert not X.verify(p("bad_instance.json"), p("model.json"), p("vk.key"), case["srs"])


@pytest.mark.parametrize("tri", [t for t in E2E if "KZGCommit" in t], ids=VC.ids)
def test_the_witness_files_commitments_are_the_proofs_first_points(root, tri):
    """the point of the feature: gen_witness's processed_*.polycommit, in the order input, params, output, ARE the proof's leading
    points; swapping them in changes nothing, swapping in those of another input (or other parameters) makes the proof invalid"""
    from ezkl_amd import execute as X
    case = _chain(root, VC.ids(tri), VC.description(tri), SRS_K6)
    p = case["p"]
    points = X.witness_commitments(p("w_host.json"))
    assert len(points) == sum(v == "KZGCommit" for v in tri) and len(set(points)) == len(points)
    assert _leading_points(case["proof_h"], len(points)) == points
    shutil.copy(p("proof_host.json"), p("swapped.json"))
    res = X.swap_proof_commitments(p("swapped.json"), p("w_host.json"))
    assert res["commitments"] == len(points) and not res["changed"] and res["proof"] == case["proof_h"]
    assert X.verify(p("swapped.json"), p("model.json"), p("vk.key"), case["srs"])
    # another witness: of another input where the input or the output is committed, of other parameters otherwise
    if tri[0] == "KZGCommit" or tri[2] == "KZGCommit":
        X.gen_witness(p("model.json"), OTHER_DATA, output=p("w_other.json"), vk_path=p("vk.key"), srs_path=case["srs"])
    else:
        weights = [list(r) for r in VC.WEIGHTS]
        weights[2][1] += 1
        open(p("other_model.json"), "w").write(json.dumps(VC.description(tri, weights=weights)))
        X.gen_witness(p("other_model.json"), DATA, output=p("w_other.json"), vk_path=p("vk.key"), srs_path=case["srs"])
    other = X.witness_commitments(p("w_other.json"))
    assert len(other) == len(points) and other != points
    shutil.copy(p("proof_host.json"), p("swapped_other.json"))
    res = X.swap_proof_commitments(p("swapped_other.json"), p("w_other.json"))
    assert res["changed"] and res["proof"][64 * len(points):] == case["proof_h"][64 * len(points):]
    assert _leading_points(res["proof"], len(points)) == other
    assert not X.verify(p("swapped_other.json"), p("model.json"), p("vk.key"), case["srs"])


def test_fixed_parameters_are_part_of_the_key(root):
    """two circuits that differ in ONE weight have different vks, and a proof made under the one key does not verify under the other"""
    from ezkl_amd import execute as X
    tri = ("Public", "Fixed", "Public")
    case = _chain(root, VC.ids(tri), VC.description(tri), SRS_K6)
    weights = [list(r) for r in VC.WEIGHTS]
    weights[2][1] += 1
    other = _chain(root, "one_weight_off", VC.description(tri, weights=weights), SRS_K6)
    assert open(case["p"]("vk.key"), "rb").read() != open(other["p"]("vk.key"), "rb").read()
    assert X.verify(other["p"]("proof_host.json"), other["p"]("model.json"), other["p"]("vk.key"), SRS_K6)
    assert not X.verify(other["p"]("proof_host.json"), case["p"]("model.json"), case["p"]("vk.key"), SRS_K6)
    assert not X.verify(case["p"]("proof_host.json"), other["p"]("model.json"), other["p"]("vk.key"), SRS_K6)


@pytest.mark.parametrize("length", [1, 57, 58, 59])
def test_a_resident_column_commits_to_what_the_host_message_commits_to(hip, golden_srs, length):
    """backend.polycommit_commit_dev against backend.polycommit_commit at k = 6, n = 2^6 - 6 = 58 values a column: one value, a full
    column less one, exactly a column (the reference then emits the extra commitment to an empty column) and one more"""
    from ezkl_amd import backend as B
    n, rows, u = 58, 64, 6
    rng = np.random.default_rng(100 + length)
    msg = rng.integers(0, 1 << 62, (length, 4), dtype=np.uint64)
    msg[:, 3] &= np.uint64((1 << 60) - 1)                                     # below r: any such word is some element's Montgomery form
    params = B.ParamsKZG(6, golden_srs["g"], golden_srs["g_lagrange"])
    cols = []
    try:
        want = B.polycommit_commit(msg, u, params)
        assert want.shape == (length // n + 1, 8)
        for j in range(length // n + 1):
            host = np.zeros((rows, 4), np.uint64)
            part = msg[j * n:(j + 1) * n]
            host[:len(part)] = part
            host[n:] = np.uint64(12345)                                       # whatever the unusable rows held is overwritten
            cols.append(B.DeviceBuffer.from_numpy(host))
        got = B.polycommit_commit_dev(cols, length, u, params)
        assert got.shape == want.shape and (got == want).all()
        assert len({bytes(p) for p in got}) == len(got)
        with pytest.raises(ValueError, match="columns"):
            B.polycommit_commit_dev(cols[:-1], length, u, params)
    finally:
        for c in cols:
            c.free()
        params.free()


def test_parameters_that_span_two_columns_end_to_end(root):
    from ezkl_amd import execute as X
    weights, biases, x, k, w = VC.two_column()
    tri = ("Private", "KZGCommit", "Public")
    srs = str(root / "kzg7.srs")
    X.gen_srs(srs, k, secret=0x5eed7)
    case = _chain(root, "two_columns", VC.description(tri, weights, biases, k, w), srs, data={"input_data": [[float(v) for v in x]]})
    p = case["p"]
    assert open(p("w_host.json"), "rb").read() == open(p("w_dev.json"), "rb").read()
    points = X.witness_commitments(p("w_host.json"))
    assert len(points) == 2 == len(case["wh"]["processed_params"]["polycommit"][0])           # 132 // 122 + 1
    assert case["proof_h"] == case["proof_d"] and _leading_points(case["proof_h"], 2) == points
    assert X.verify(p("proof_dev.json"), p("model.json"), p("vk.key"), srs) and X.mock(p("w_host.json"), p("model.json")) == ""


def test_a_session_on_committed_parameters(root):
    """two witnesses through one Prover: both proofs verify and carry the same parameter commitment, the witness files' own"""
    from ezkl_amd import execute as X
    tri = ("Public", "KZGCommit", "Public")
    case = _chain(root, VC.ids(tri), VC.description(tri), SRS_K6)
    p = case["p"]
    X.gen_witness(p("model.json"), OTHER_DATA, output=p("w2.json"), vk_path=p("vk.key"), srs_path=SRS_K6, synthesis="device", pk_path=p("pk.key"))
    proofs = []
    with X.Prover(p("model.json"), p("pk.key"), SRS_K6, synthesis="device") as session:
        for i, wit in enumerate((p("w_host.json"), p("w2.json"))):
            how = {}
            proofs.append(session.prove(wit, p("session%d.json" % i), seed=SEED + i, report=how))
            assert how["path"] == "device"
            assert X.verify(p("session%d.json" % i), p("model.json"), p("vk.key"), SRS_K6)
    assert proofs[0] != proofs[1]
    commitment = X.witness_commitments(p("w_host.json"))
    assert len(commitment) == 1 and commitment == X.witness_commitments(p("w2.json"))
    assert _leading_points(proofs[0], 1) == _leading_points(proofs[1], 1) == commitment
