"""The SRS point predicate (ezkl_amd/csrc/srs_check.hpp: is a 64-byte record of the file a point of G1, as halo2's raw-bytes reader decides
it) built as a plain program under AddressSanitizer and UndefinedBehaviorSanitizer and held, case by case, to its restatement in Python
integers (tests/srs_check_ref.py): tests/cpp/test_srs_check.cpp reads the cases this file writes.  No device, no library loaded into the
interpreter, no preload."""
import os
import subprocess

import numpy as np

import srs_check_ref as CR
from conftest import GOLDEN, ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "test_srs_check.cpp")
_FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "ezkl_amd", "csrc"), SRC]
Q, MONT = CR.Q, CR.MONT


def _run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, **kw)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    return r


def cases():
    """[(name, record)]: the edge cases of the predicate, then every point of the golden k = 6 file"""
    G = (1, 2)
    G2 = CR.double(*G)
    out = [("generator", CR.affine(*G)), ("2G", CR.affine(*G2)), ("-G", CR.affine(1, Q - 2)), ("identity", CR.record(0, 0))]
    # x = q - 1, as the stored word and as the canonical value, with the matching y where one exists (else y = 1: off the curve)
    for name, x in (("stored x = q - 1", (Q - 1) * CR.RINV % Q), ("canonical x = q - 1", Q - 1)):
        y = CR.sqrt(x ** 3 + 3)
        out.append((name + (" with its y" if y is not None else ", no y exists"), CR.affine(x, y if y is not None else 1)))
    good_y = 2 * MONT % Q
    out += [("x = q", CR.record(Q, good_y)), ("x = 2^256 - 1", CR.record((1 << 256) - 1, good_y)), ("y = q", CR.record(MONT % Q, Q)),
            ("y = 2^256 - 1", CR.record(MONT % Q, (1 << 256) - 1)), ("both bad: reason 1", CR.record(Q + 5, Q + 9)),
            ("x = q, y zero", CR.record(Q, 0)), ("x zero, y = q", CR.record(0, Q))]
    xw, yw = CR.words(CR.affine(*G2))
    for limb in range(8):                                # a valid point with one bit of y flipped, in every limb
        out.append(("2G, bit %d of y flipped" % (32 * limb + 5), CR.record(xw, yw ^ (1 << (32 * limb + 5)))))
        out.append(("2G, bit %d of x flipped" % (32 * limb + 30), CR.record(xw ^ (1 << (32 * limb + 30)), yw)))
    out += [("(0, 1)", CR.affine(0, 1)), ("(1, 0)", CR.affine(1, 0)), ("words (0, 1)", CR.record(0, 1)), ("words (1, 0)", CR.record(1, 0))]
    out += [("bad_point(%d)" % why, CR.bad_point(why)) for why in (1, 2, 3)]
    buf = open(os.path.join(GOLDEN, "kzg_k6.srs"), "rb").read()
    pts = np.frombuffer(buf, np.uint64, count=8 * 128, offset=4).reshape(128, 8)
    out += [("kzg_k6.srs point %d" % i, pts[i]) for i in range(128)]
    return out


def test_the_reference_itself_on_known_points():
    """srs_check_ref before it judges anything: the generator and its double are on the curve, the golden file's points are all valid,
    each planted reason is the one asked for, and both-bad answers 1"""
    got = {name: CR.reason(p) for name, p in cases()}
    assert got["generator"] == got["2G"] == got["-G"] == (0, False) and got["identity"] == (0, True)
    assert all(v == (0, False) for name, v in got.items() if name.startswith("kzg_k6"))
    assert [got["bad_point(%d)" % w][0] for w in (1, 2, 3)] == [1, 2, 3]
    assert got["both bad: reason 1"][0] == 1 and got["x = q"][0] == 1 and got["y = q"][0] == 2 and got["x zero, y = q"][0] == 2
    assert got["(0, 1)"][0] == got["(1, 0)"][0] == 3
    flipped = [v[0] for name, v in got.items() if "flipped" in name]
    assert len(flipped) == 16 and all(flipped)
    assert any("with its y" in name and v == (0, False) for name, v in got.items())


def test_srs_point_predicate_under_the_sanitizers(tmp_path):
    exe, path = str(tmp_path / "test_srs_check"), str(tmp_path / "cases.bin")
    cs = cases()
    with open(path, "wb") as f:
        for _, p in cs:
            r, ident = CR.reason(p)
            f.write(np.asarray(p, np.uint64).tobytes() + bytes([r | (4 if ident else 0)]))
    _run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] + _FLAGS + ["-o", exe])
    r = _run([exe, path], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert "%d cases:" % len(cs) in r.stdout and "all checks passed" in r.stdout
    for mark in ("Sanitizer", "runtime error"):
        assert mark not in r.stderr, r.stderr[-6000:]
