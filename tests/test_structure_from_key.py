"""`execute.prove` / `execute.verify` take the constraint system from the KEY FILE, not from a layout of the circuit: halo2's vk.key
(the prefix of pk.key) carries every selector's rows bit-packed, and `configure` + selector compression on those rows is the system
keygen saw (execute._plonk_cs; halo2 does the same on load_pk).  Checked against the layout (execute._fresh_keygen_inputs, what `setup`
and `mock` still run) on the reference's own k = 6 key files and on k = 8 / k = 10 MLPs whose rows are packed as
NativeProvingKey.set_selectors packs them; `verify` is then run with the layout engine disabled."""
import os
import pickle
import struct
import sys

import numpy as np
import pytest

import fixture_k6 as FX
from test_ezkl_circuit import FIXTURE_B, FIXTURE_W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_system(got, want):
    for name in ("k", "n_advice", "n_fixed", "n_selectors", "n_instance", "perm", "degree", "ext_k", "advice_queries", "fixed_queries",
                 "instance_queries"):
        assert getattr(got, name) == getattr(want, name), name
    assert pickle.dumps(got.gates) == pickle.dumps(want.gates), "gates"
    assert pickle.dumps(got.lookups) == pickle.dumps(want.lookups), "lookups"


def _layout(circuit):
    """(the layout's constraint system, a vk.key of it: zero commitments, selector rows as set_selectors packs them)"""
    from ezkl_amd import execute as X
    cs, _, _, reg = X._fresh_keygen_inputs(circuit)
    bits = np.packbits(np.asarray(reg.selector_rows(), bool), axis=1, bitorder="little").tobytes()
    return cs, bytes([3, circuit.k, 1]) + struct.pack("<I", cs.n_fixed) + bytes(64 * (cs.n_fixed + len(cs.perm))) + bits


def _mlp(k, weights, biases):
    from ezkl_amd import ezkl_layout as EL
    return EL.MlpCircuit(k, 2, weights, biases, 128, 2)


@pytest.fixture(scope="module")
def golden_circuit():
    from ezkl_amd import execute as X
    circuit, _ = X._load_circuit(os.path.join(FX.G, "model_k6.compiled"))
    return circuit, X._fresh_keygen_inputs(circuit)[0]


def test_system_from_the_reference_vk_file_equals_the_layouts(golden_circuit):
    from ezkl_amd import execute as X
    circuit, want = golden_circuit
    _same_system(X._plonk_cs(circuit, os.path.join(FX.G, "vk_k6.key")), want)
    _same_system(X._plonk_cs(circuit, open(os.path.join(FX.G, "vk_k6.key"), "rb").read()), want)       # the bytes work as the path does
    assert want.n_fixed == 38 and want.n_selectors == 80 and len(want.perm) == 32


def test_system_from_the_reference_pk_file_reads_only_its_vk_prefix(golden_circuit, monkeypatch):
    from ezkl_amd import execute as X
    circuit, want = golden_circuit
    path, read = os.path.join(FX.G, "pk_k6.key"), []

    class Counting:
        def __init__(self, f): self.f = f
        def read(self, *a):
            b = self.f.read(*a)
            read.append(len(b))
            return b
        def __getattr__(self, name): return getattr(self.f, name)
        def __enter__(self): return self
        def __exit__(self, *exc): self.f.close()

    monkeypatch.setattr(X, "open", lambda p, *a, **kw: Counting(open(p, *a, **kw)) if p == path else open(p, *a, **kw), raising=False)
    _same_system(X._plonk_cs(circuit, path), want)
    vk_len = os.path.getsize(os.path.join(FX.G, "vk_k6.key"))
    assert vk_len == 5127 and sum(read) == vk_len < os.path.getsize(path)


@pytest.mark.parametrize("k", [8, 10])
def test_system_from_packed_selector_rows_equals_the_layouts(k):
    """k = 8: the fixture model; k = 10: the bench MLP (9 layers, two blocks of advice columns), both with base 128"""
    from ezkl_amd import execute as X
    if k == 8:
        circuit = _mlp(8, [FIXTURE_W], [FIXTURE_B])
    else:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import bench_circuits as BC
        circuit, _ = BC.mlp_circuit(10, np.random.default_rng(1), base=128)
    want, key = _layout(circuit)
    _same_system(X._plonk_cs(circuit, key), want)
    _same_system(X._plonk_cs(circuit, key + b"\x07" * 100), want)               # a pk.key goes on after the vk
    assert circuit.gc.cs.selectors and not hasattr(circuit.gc.cs, "selector_map"), "the loaded circuit's own system is left as configured"


@pytest.fixture(scope="module")
def golden_proof(tmp_path_factory):
    """a proof of the reference's witness on the reference's circuit under the k = 6 test SRS, made on the CPU (the Python prover on the
    oracle backend, as tests/test_ezkl_circuit.py makes it), with the vk.key of that keygen: the selector rows are the reference key's"""
    from ezkl_amd import codecs, plonk as P
    from oracle import pyref as pr
    from oracle.cpu_backend import OracleBackend
    d = tmp_path_factory.mktemp("verify")
    fx = FX.load()
    srs = pr.parse_srs(open(os.path.join(FX.G, "kzg_k6.srs"), "rb").read())
    g, gl = (np.stack([np.frombuffer(b, np.uint64) for b in srs[name]]) for name in ("g", "g_lagrange"))
    be = OracleBackend(g, gl, FX.K)
    adv, inst, _ = FX.witness(fx)
    pk, vk = P.keygen(fx["cs"], be, FX.mont_cols(fx["fixed"]), FX.copies_of(FX.copy_cycles(fx["pk"])))
    pk.vk, pk.selectors = vk, fx["pk"]["vk"]["selectors"]
    proof = P.create_proof(pk, be, FX.mont_cols(adv), P.Rng(7), instances=inst)
    (d / "vk.key").write_bytes(P.export_keys(pk, be)[0])
    (d / "proof.json").write_text(codecs.write_proof_json(proof, inst))
    return d, proof, inst


def test_verify_lays_nothing_out(golden_proof, monkeypatch):
    """the test that fails without the change: `verify` with the layout engine's synthesis disabled"""
    from ezkl_amd import codecs, execute as X, ezkl_layout as EL
    d, proof, inst = golden_proof
    def no_layout(self, *a, **kw):
        raise AssertionError("verify laid the circuit out")
    monkeypatch.setattr(EL.MlpCircuit, "synthesize", no_layout)
    compiled, srs = os.path.join(FX.G, "model_k6.compiled"), os.path.join(FX.G, "kzg_k6.srs")
    assert X.verify(str(d / "proof.json"), compiled, str(d / "vk.key"), srs)
    bad = bytearray(proof); bad[4000] ^= 1
    (d / "bad.json").write_text(codecs.write_proof_json(bytes(bad), inst))
    assert not X.verify(str(d / "bad.json"), compiled, str(d / "vk.key"), srs)
    (d / "other.json").write_text(codecs.write_proof_json(proof, [[1, 0, 0, 0]]))
    assert not X.verify(str(d / "other.json"), compiled, str(d / "vk.key"), srs)          # other public outputs
    with pytest.raises(ValueError, match="recommit=True needs the PROVING key"):          # decided from the key's own length, before any device work
        X.verify(str(d / "proof.json"), compiled, str(d / "vk.key"), srs, recommit=True)


def test_a_key_of_another_circuit_and_a_short_key_are_refused(tmp_path):
    """same k, other layer widths: 12 outputs need a second block of advice columns, so the layouts differ in their selectors and in
    the fixed columns these compress to -- which is what the key is checked by (a key whose counts all agree is the same constraint
    system, and a proof under it simply does not verify)"""
    from ezkl_amd import execute as X
    mine, other = _mlp(8, [FIXTURE_W], [FIXTURE_B]), _mlp(8, [[[1, 0, 0]] * 12], [[0] * 12])
    (cs_mine, key_mine), (cs_other, key_other) = _layout(mine), _layout(other)
    assert cs_mine.n_fixed != cs_other.n_fixed
    with pytest.raises(ValueError, match="does not belong to this circuit"):
        X._plonk_cs(mine, key_other)
    (tmp_path / "other.key").write_bytes(key_other)
    with pytest.raises(ValueError, match="does not belong to this circuit"):
        X._plonk_cs(mine, str(tmp_path / "other.key"))
    with pytest.raises(ValueError, match="does not belong to this circuit"):
        X._plonk_cs(mine, _layout(_mlp(9, [FIXTURE_W], [FIXTURE_B]))[1])
    for short in (key_mine[:100], key_mine[:5], key_mine[:-1]):
        with pytest.raises(RuntimeError, match="truncated"):
            X._plonk_cs(mine, short)
    (tmp_path / "short.key").write_bytes(key_mine[:100])
    with pytest.raises(RuntimeError, match="truncated"):
        X._plonk_cs(mine, str(tmp_path / "short.key"))
    _same_system(X._plonk_cs(mine, key_mine), cs_mine)
