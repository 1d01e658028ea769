"""Compressed G1 points on the device (ezkl_amd/csrc/g1_compress.hip: g1_decompress_kernel, one square root in Fq per lane by a generated
exponent chain, and g1_compress_kernel) against the Python integers of tests/g1_compress_ref.py, word for word; the refusals with their
lowest index and reason; and processed SRS files through every loader of ezkl_amd.execute."""
import json
import os

import numpy as np
import pytest

import fixture_k6 as FX
import g1_compress_ref as GR
from conftest import Q, rand_fr
from test_ezkl_circuit import FIXTURE_B, FIXTURE_W
from test_g1_compress_cpu import NON_RESIDUE_X

pytestmark = pytest.mark.gpu
SIZES = [1, 63, 64, 65, 257, 4097]          # one lane, a partial wave, a full one, one lane past it, past one and several workgroups
SRS = os.path.join(FX.G, "kzg_k6.srs")


@pytest.fixture(scope="module")
def points():
    """(records, their negatives): at every index both sign bits occur, one in each set"""
    pts = GR.multiples(max(SIZES), 20261126)
    neg = np.array([GR.affine(x, Q - y) for x, y in ((xw * GR.RINV % Q, yw * GR.RINV % Q) for xw, yw in map(GR.words, pts))])
    return pts, neg


def _enc(records):
    return b"".join(GR.compress(p) for p in records)


@pytest.mark.parametrize("n", SIZES)
def test_decompress_and_back_against_the_reference(hip, points, n):
    from ezkl_amd import backend as B
    signs = []
    for records in points:
        data = _enc(records[:n])
        signs.append(np.frombuffer(data, np.uint8)[31::32] >> 6)
        b = B.Bases.from_compressed(data)
        try:
            assert b.n == n and b.download().tobytes() == records[:n].tobytes()
            assert b.compressed() == data
        finally:
            b.free()
        assert B.last_kernel_ms("g1_decompress") > 0
    assert ((signs[0] ^ signs[1]) == 1).all()


def test_msm_of_a_decompressed_set_is_the_msm_of_the_raw_upload(hip, points):
    from ezkl_amd import backend as B
    n = 257
    records = points[0][:n].copy()
    records[100] = 0                                                           # an identity in the middle: accepted, and the MSM ignores it
    data = _enc(records)
    assert data[32 * 100:32 * 101] == GR.IDENTITY
    a, b, d = B.Bases.from_compressed(data), B.Bases(records), B.DeviceBuffer.from_numpy(rand_fr(np.random.default_rng(3), n))
    try:
        assert a.download().tobytes() == records.tobytes()
        assert a.msm_once(d.ptr).tobytes() == b.msm_once(d.ptr).tobytes()
        s = d.to_numpy(shape=(n, 4))
        s[100] = 0                                                             # whatever its scalar: the identity adds nothing
        z = B.DeviceBuffer.from_numpy(s)
        assert a.msm_once(d.ptr).tobytes() == b.msm_once(z.ptr).tobytes()
        z.free()
    finally:
        a.free(); b.free(); d.free()


BAD = {"non-residue": (NON_RESIDUE_X.to_bytes(32, "little"), 3), "x = p": (Q.to_bytes(32, "little"), 1),
       "x = 2^254 - 1": (((1 << 254) - 1).to_bytes(32, "little"), 1), "identity flag, x = 1": ((1 << 255 | 1).to_bytes(32, "little"), 4)}


@pytest.mark.parametrize("where", [0, 64, 129])
@pytest.mark.parametrize("kind", sorted(BAD))
def test_bad_encodings_are_refused_with_index_and_reason(hip, points, kind, where):
    from ezkl_amd import backend as B, lib as L
    import ctypes as C
    enc, why = BAD[kind]
    assert GR.decompress(enc) == (None, why)
    data = bytearray(_enc(points[0][:130]))
    data[32 * where:32 * where + 32] = enc
    with pytest.raises(B.CompressedPointError) as e:
        B.Bases.from_compressed(bytes(data), "g")
    assert (e.value.index, e.value.reason) == (where, why) and str(e.value).startswith("g[%d]: " % where)
    if where:                                                                  # a second bad point below it: index and reason are the lower one's
        other = BAD["x = p" if kind != "x = p" else "non-residue"]
        data[32:64] = other[0]
        with pytest.raises(B.CompressedPointError) as e:
            B.Bases.from_compressed(bytes(data))
        assert (e.value.index, e.value.reason) == (1, other[1])
    h, bad, reason = C.c_void_p(0x1234), C.c_uint64(0), C.c_int(0)             # the output handle is untouched
    a = np.frombuffer(bytes(data), np.uint8)
    assert L.load().ezkl_hip_bases_decompress(a.ctypes.data_as(C.c_void_p), C.c_size_t(130), C.byref(h), C.byref(bad), C.byref(reason)) == 0
    assert h.value == 0x1234 and reason.value != 0


def test_processed_srs_file_through_the_loaders(hip, tmp_path, monkeypatch):
    from ezkl_amd import codecs, execute as X
    packed, back = str(tmp_path / "kzg_k6.processed.srs"), str(tmp_path / "kzg_k6.raw.srs")
    info = X.compress_srs(SRS, packed)
    assert info["k"] == 6 and os.path.getsize(packed) == 4 + 64 * 64 + 128
    assert X.decompress_srs(packed, back)["sha256_out"] == info["sha256_in"] and open(back, "rb").read() == open(SRS, "rb").read()
    monkeypatch.setenv("EZKL_SRS_CHECK", "full")
    assert X.check_srs(packed)["ok"]
    st = json.load(open(os.path.join(FX.G, "settings_k6.json")))
    compiled = tmp_path / "model.compiled.json"
    compiled.write_text(json.dumps({"model": "mlp", "run_args": st["run_args"], "weights": [FIXTURE_W], "biases": [FIXTURE_B],
                                    "total_assignments": st["total_assignments"]}))
    proofs = {}
    for name, srs in (("raw", SRS), ("processed", packed)):
        vk, pk, pr = (str(tmp_path / (name + ext)) for ext in (".vk", ".pk", ".proof.json"))
        X.setup(str(compiled), srs, vk, pk)
        proofs[name] = X.prove(os.path.join(FX.G, "witness_k6.json"), str(compiled), pk, pr, srs, X.CheckMode.SAFE, seed=42)
        assert X.verify(pr, str(compiled), vk, srs)
    assert proofs["raw"] == proofs["processed"]
    monkeypatch.setenv("EZKL_SRS_CHECK", "points")
    buf = bytearray(open(packed, "rb").read())
    for name, index in (("g", 13), ("g_lagrange", 7)):
        off = 4 + (32 * 64 if name == "g_lagrange" else 0) + 32 * index
        x = int.from_bytes(buf[off:off + 32], "little")
        bit = next(b for b in range(8) if GR.decompress((x ^ 1 << b).to_bytes(32, "little"))[1] == 3)   # a flip that leaves no point
        damaged = bytearray(buf)
        damaged[off] ^= 1 << bit
        path = tmp_path / ("damaged_%s.srs" % name)
        path.write_bytes(bytes(damaged))
        with pytest.raises(X.SrsError, match=r"^%s\[%d\]: no point with this x" % (name, index)):
            X.check_srs(str(path), structure=False)
    assert codecs.read_srs_g2(packed) == codecs.read_srs_g2(SRS)
