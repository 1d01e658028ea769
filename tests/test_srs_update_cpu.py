"""The SRS update without a device: what execute.update_srs refuses before it touches a file or a library, where the new symbol is
declared, and the one verdict of verify_srs_update that is decided on the host alone (files of different k)."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, R, ROOT


@pytest.fixture()
def no_library(monkeypatch):
    """either library's loader raises: a test that passes under this fixture has not asked for one"""
    from ezkl_amd import lib as L, native as NV

    def refuse(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(L, "load", refuse)
    monkeypatch.setattr(NV, "load", refuse)


@pytest.mark.parametrize("secret", [0, -1, -R, R, R + 1, 1 << 256, 1.5, 7.0, "7", b"\x07", True, np.float64(3)],
                         ids=["zero", "minus_one", "minus_r", "r", "r_plus_one", "2^256", "fraction", "float", "str", "bytes", "bool", "np_float"])
def test_update_srs_refuses_a_secret_outside_1_to_r_before_anything_else(no_library, tmp_path, secret):
    """ValueError about the secret: not FileNotFoundError about the input (it does not exist), not the loader's AssertionError, and no
    output file"""
    from ezkl_amd import execute as X
    out = tmp_path / "out.srs"
    with pytest.raises(ValueError, match=r"the secret must be an integer in \[1, r\)"):
        X.update_srs(str(tmp_path / "no_such_file.srs"), str(out), secret=secret)
    assert not out.exists()


def test_backend_update_srs_refuses_the_same_secrets(no_library):
    from ezkl_amd import backend as B
    for secret in (0, -1, R, 2.0, None):
        with pytest.raises(ValueError, match=r"the secret must be an integer in \[1, r\)"):
            B.update_srs(dict(k=6), secret)


def test_an_accepted_secret_reaches_the_input_file(no_library, tmp_path):
    """1, r - 1 and numpy integers pass the secret check: the next thing that fails is the missing input"""
    from ezkl_amd import execute as X
    for secret in (1, R - 1, np.int64(5), np.uint64(5)):
        with pytest.raises(FileNotFoundError):
            X.update_srs(str(tmp_path / "no_such_file.srs"), str(tmp_path / "out.srs"), secret=secret)


def test_a_drawn_secret_is_in_range(monkeypatch):
    from ezkl_amd import execute as X
    draws = [bytes(64), (R).to_bytes(64, "little"), (2 * R + 5).to_bytes(64, "little")]          # 0 and r reduce to 0: redrawn
    monkeypatch.setattr(X.os, "urandom", lambda n: draws.pop(0) if n == 64 else 1 / 0)
    assert X._update_secret(None) == 5 and not draws
    monkeypatch.undo()
    assert all(1 <= X._update_secret(None) < R for _ in range(8))


def test_the_symbol_is_in_the_loaders_list_and_in_the_header():
    from ezkl_amd import lib as L
    assert L.SYMBOLS.count("ezkl_hip_bases_mul_scalars") == 1
    header = open(os.path.join(ROOT, "include", "ezkl_hip.h")).read()
    decl = re.search(r"^int ezkl_hip_bases_mul_scalars\(ezkl_bases_t \w+, const void\* \w+, size_t first, size_t n, ezkl_bases_t\* \w+\);$", header, re.M)
    assert decl, "include/ezkl_hip.h does not declare ezkl_hip_bases_mul_scalars with the documented signature"
    assert header.index("int ezkl_hip_bases_from_scalars(") < decl.start() < header.index("int ezkl_hip_bases_downsize(")   # next to from_scalars
    assert L.load().ezkl_hip_bases_mul_scalars                                   # and the built library exports it


def test_a_null_handle_or_an_empty_range_is_refused_before_the_device_is_asked_for():
    import ctypes as C
    from ezkl_amd import lib as L
    h, one = C.c_void_p(), C.c_void_p(1)
    f = L.load().ezkl_hip_bases_mul_scalars
    assert f(None, one, C.c_size_t(0), C.c_size_t(1), C.byref(h)) == -3
    assert f(one, None, C.c_size_t(0), C.c_size_t(1), C.byref(h)) == -3
    assert f(one, one, C.c_size_t(0), C.c_size_t(0), C.byref(h)) == -3           # n = 0: a base set is never empty
    assert f(one, one, C.c_size_t(0), C.c_size_t(1), None) == -3
    assert h.value is None


def _golden(name):
    from ezkl_amd import codecs
    return codecs.read_srs(open(os.path.join(GOLDEN, name), "rb").read())


def test_files_of_different_k_are_told_apart_without_a_device(no_library, tmp_path):
    from ezkl_amd import backend as B, execute as X
    old, new = _golden("kzg_k6.srs"), _golden("kzg_k1_public.srs")
    for a, b, ka, kb in ((old, new, 6, 1), (new, old, 1, 6)):
        rep = B.verify_srs_update(a, b, dict(t_g2=bytes(128)))
        assert rep == dict(k=None, old=None, new=None, t_g2=None, link=None, ok=False,
                           reason="k: the old file has k = %d, the new one k = %d" % (ka, kb))
    with pytest.raises(X.SrsError, match=r"^k: the old file has k = 6, the new one k = 1$") as e:
        X.verify_srs_update(os.path.join(GOLDEN, "kzg_k6.srs"), os.path.join(GOLDEN, "kzg_k1_public.srs"), "00" * 128)
    assert e.value.report["ok"] is False and e.value.report["old"] is None


def test_a_different_g2_and_a_different_first_point_are_told_on_the_host(no_library):
    from ezkl_amd import backend as B
    old = _golden("kzg_k6.srs")
    twisted = bytearray(old["g2"]); twisted[0] ^= 1
    rep = B.verify_srs_update(old, dict(old, g2=bytes(twisted)), dict(t_g2=bytes(128)))
    assert not rep["ok"] and rep["k"] == 6 and rep["reason"].startswith("g2:") and rep["old"] is None
    g = old["g"].copy(); g[0] = g[1]
    rep = B.verify_srs_update(old, dict(old, g=g), dict(t_g2=bytes(128)))
    assert not rep["ok"] and rep["reason"].startswith("g[0]:") and rep["old"] is None
