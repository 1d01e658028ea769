"""Compressed G1 points without a device: the Python reference (tests/g1_compress_ref.py) against the golden k = 6 SRS, the processed file
layout of ezkl_amd.codecs, the host Fq2 square root behind its two G2 points, the generated exponent chain of the device's square root
(tools/gen_fq_sqrt_chain.py) against pow(), and the encoding table (csrc/g1_encoding.hpp) as a plain program under ASan + UBSan."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import g1_compress_ref as GR
from conftest import GOLDEN, Q, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_fq_sqrt_chain as GEN  # noqa: E402

NON_RESIDUE_X = next(x for x in range(2, 100) if GR.decompress(x.to_bytes(32, "little"))[1] == 3)


def test_reference_round_trip_on_the_golden_srs(golden_srs):
    for rec in np.concatenate([golden_srs["g"], golden_srs["g_lagrange"]]):
        back, why = GR.decompress(GR.compress(rec))
        assert why == 0 and back.tobytes() == rec.tobytes()
    assert GR.decompress(GR.compress(np.zeros(8, np.uint64))) [0].tobytes() == bytes(64)


def test_codecs_round_trip_a_processed_file(golden_srs):
    from ezkl_amd import codecs
    raw = codecs.read_srs(golden_srs["buf"])
    packed = dict(raw, **{name: np.frombuffer(b"".join(GR.compress(p) for p in raw[name]), np.uint8).reshape(-1, 32) for name in ("g", "g_lagrange")})
    data = codecs.write_srs(packed)
    assert len(data) == 4 + 64 * 64 + 128 == codecs._srs_len_processed(6)
    back = codecs.read_srs(data)
    assert codecs.srs_is_processed(back) and not codecs.srs_is_processed(raw) and back["k"] == 6
    assert all(back[name].tobytes() == packed[name].tobytes() for name in ("g", "g_lagrange"))
    assert back["g2"] == raw["g2"] and back["s_g2"] == raw["s_g2"]
    for damaged in (data[:-1], data + b"\0", data[:4 + 32 * 64]):             # any other length: refused with the raw reader's words
        with pytest.raises(ValueError, match="SRS length %d does not match k=6" % len(damaged)):
            codecs.read_srs(damaged)


def test_host_fq2_root_on_the_files_g2_points(golden_srs):
    from ezkl_amd import codecs
    raw = codecs.read_srs(golden_srs["buf"])
    for name in ("g2", "s_g2"):
        assert codecs.g2_decompress(codecs.g2_compress(raw[name])) == raw[name]
        flipped = bytearray(codecs.g2_compress(raw[name]))
        flipped[63] ^= 0x40                                                    # the other sign: the other root, y -> -y
        x0, x1, y0, y1 = (int.from_bytes(raw[name][i:i + 32], "little") for i in range(0, 128, 32))
        neg = codecs.g2_decompress(bytes(flipped))
        assert neg[:64] == raw[name][:64] and [int.from_bytes(neg[i:i + 32], "little") for i in (64, 96)] == [Q - y0, Q - y1]
    rng = random.Random(5)
    for _ in range(20):
        a = (rng.randrange(Q), rng.randrange(Q))
        sq = ((a[0] * a[0] - a[1] * a[1]) % Q, 2 * a[0] * a[1] % Q)
        r = codecs.fq2_sqrt(sq)
        assert r in (a, (Q - a[0], Q - a[1]))
    assert codecs.fq2_sqrt((4, 0)) in ((2, 0), (Q - 2, 0)) and codecs.fq2_sqrt((Q - 4, 0)) in ((0, 2), (0, Q - 2))


@pytest.mark.parametrize("window", [GEN.WINDOW, 1])
def test_generated_exponent_chain_equals_pow(window):
    ops = GEN.chain(GEN.E, window)
    rng = random.Random(7)
    non_residue = (NON_RESIDUE_X ** 3 + 3) % Q
    assert pow(non_residue, (Q - 1) // 2, Q) == Q - 1
    for t in [0, 1, Q - 1, non_residue] + [rng.randrange(Q) for _ in range(100)]:
        assert GEN.evaluate(ops, t, Q, window) == pow(t, (Q + 1) // 4, Q)
    header = open(os.path.join(ROOT, "ezkl_amd", "csrc", "fq_sqrt_chain_gen.hpp")).read()
    assert header == GEN.emit()                                                # the committed header is what the generator emits


def test_encoding_table_under_the_sanitizers(tmp_path, golden_srs):
    exe, path = str(tmp_path / "test_g1_encoding"), str(tmp_path / "cases.bin")
    cases = [GR.compress(p) for p in golden_srs["g"]] + [GR.IDENTITY]
    cases += [v.to_bytes(32, "little") for v in (Q, Q - 1, (1 << 254) - 1, Q | 1 << 254, 1 << 255 | 1, 3 << 254, (1 << 256) - 1, 0, 1 << 254)]
    with open(path, "wb") as f:
        for b in cases:
            v = int.from_bytes(b, "little")
            sign, ident, x = (v >> 254) & 1, v >> 255, v & ((1 << 254) - 1)
            verdict = (4 if x or sign else 0) if ident else (1 if x >= Q else 0)
            f.write(b + bytes([verdict, sign | ident << 1]))
    src = os.path.join(ROOT, "tests", "cpp", "test_g1_encoding.cpp")
    for cmd in (["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-std=c++17", "-Wall",
                 "-Wextra", "-Werror", "-I", os.path.join(ROOT, "ezkl_amd", "csrc"), src, "-o", exe], [exe, path]):
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    assert "%d cases: all checks passed" % len(cases) in r.stdout
