"""The host-only part of the prover (prover/cs.hpp, keyfile.hpp, verify.hpp and witness_plan.hpp: the code that reads circuit blobs, key
files, proofs and witness plans from outside) built as a plain program under AddressSanitizer and UndefinedBehaviorSanitizer and run on
the k = 6 fixture: tests/cpp/test_host_prover.cpp says what it asserts.  No device, no library loaded into the interpreter, no preload."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import fixture_k6 as FX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_host_prover.cpp")
# The sanitized run (test_host_prover_under_the_sanitizers) does every truncation, every bit flip in the proof's 114 points, the vk's
# header and commitments; its single-byte sweeps of the 91 KB circuit blob visit every STRIDE-th byte (61: coprime to the blob's 4-byte
# words and 48-byte node records, so every byte position of both is visited), the flips in the vk's selector section every STRIDE-th bit.
# Of the 59 136 evaluation bits of the proof (231 evaluations) it flips every EVAL_STEP-th, one in each evaluation at a bit position that
# moves along: a flipped evaluation is rejected only by the pairing at the very end, a whole verification of about a second under the
# sanitizers.  ALL of them are flipped by test_every_evaluation_bit_flip_is_rejected, from a build of the same program at -O2 without
# the sanitizers.  Neither is hung: on 8 cores the sanitized test takes about 3.5 minutes (35 s to
# compile, 165 s to run, 96 s of that the blob's 91 240 truncations, each of which hashes its prefix), the complete evaluation sweep about
# 20 minutes (1170 s: 0.16 s per verification).
STRIDE, EVAL_STEP = 61, 257
_FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "ezkl_amd", "csrc", "prover"), SRC]


def _inputs(d):
    """the golden_proof recipe of tests/test_structure_from_key.py: the Python prover on the oracle backend under the k = 6 test SRS"""
    from ezkl_amd import execute as X, plonk as P, witness_plan as WP
    from oracle import pyref as pr
    from oracle.cpu_backend import OracleBackend
    fx = FX.load()
    buf = open(os.path.join(FX.G, "kzg_k6.srs"), "rb").read()
    srs = pr.parse_srs(buf)
    g, gl = (np.stack([np.frombuffer(b, np.uint64) for b in srs[name]]) for name in ("g", "g_lagrange"))
    be = OracleBackend(g, gl, FX.K)
    adv, inst, _ = FX.witness(fx)
    pk, vk = P.keygen(fx["cs"], be, FX.mont_cols(fx["fixed"]), FX.copies_of(FX.copy_cycles(fx["pk"])))
    pk.vk, pk.selectors = vk, fx["pk"]["vk"]["selectors"]
    proof = P.create_proof(pk, be, FX.mont_cols(adv), P.Rng(7), instances=inst)
    circuit, _ = X._load_circuit(os.path.join(FX.G, "model_k6.compiled"))
    cs, vk_bytes = X._key_system(circuit, P.export_keys(pk, be)[0])          # the system `verify` parses, from the key alone
    put = lambda name, data: open(os.path.join(d, name), "wb").write(data)
    put("cs.blob", P.serialize_cs(cs))
    put("vk.key", vk_bytes)
    put("proof.bin", bytes(proof))
    put("instances.bin", struct.pack("<I", len(inst)) + b"".join(
        struct.pack("<I", len(col)) + b"".join(P.to_mont(v).tobytes() for v in col) for col in inst))
    put("g2.bin", buf[-256:-128])
    put("s_g2.bin", buf[-128:])
    for name in ("pk_k6.key", "vk_k6.key"):
        shutil.copy(os.path.join(FX.G, name), os.path.join(d, name))
    z = np.load(os.path.join(FX.G, "pk_k6_subset.npz"))
    put("fixed_values.bin", np.ascontiguousarray(z["fixed_values"]).tobytes())
    put("fixed_idx.bin", np.asarray(z["fixed_idx"], "<u4").tobytes())
    put("plan.blob", WP.record_plan(circuit).to_bytes())


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("host_prover"))
    _inputs(d)
    return d


def _run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, **kw)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    return r


def test_host_prover_under_the_sanitizers(inputs, tmp_path):
    exe = str(tmp_path / "test_host_prover")
    _run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] + _FLAGS + ["-o", exe])
    r = _run([exe, inputs, str(STRIDE), str(EVAL_STEP)], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert "all checks passed" in r.stdout
    for mark in ("Sanitizer", "runtime error"):
        assert mark not in r.stderr, r.stderr[-6000:]


def test_every_evaluation_bit_flip_is_rejected(inputs, tmp_path):
    """the complete sweep the sanitized run thins: 59 136 proofs with one evaluation bit flipped, each verified to the pairing"""
    exe = str(tmp_path / "test_host_prover_o2")
    _run(["g++", "-O2", "-pthread"] + _FLAGS + ["-o", exe])
    r = _run([exe, inputs, "evaluations"])
    assert "all checks passed" in r.stdout and "59136 cases" in r.stdout
