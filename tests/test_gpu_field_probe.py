"""Every field primitive of csrc/field.hpp (radix 2^32, Fr and Fq) and csrc/field29.hpp (radix 2^29, Fr29 and Fq29) on the device, one at
a time (ezkl_hip_field_probe_dev, csrc/fieldprobe.hip), against Python integers (tests/field_edge_ref.py), word for word: operands
with limbs of 0, 0xffffffff and 2^29 - 1 and values on p, 2p and K p, where a wrong carry, borrow or conditional subtraction shows and
where random residues never land.  The expectations are exact words, not congruences: a lazily reduced result that is off by p fails.

The live-register probes run each inline-assembly product with six further operand rows and 64 uniform words held in registers across
it and expect them back unchanged: the only check that a clobber list is complete.

tests/test_field_edge_ref.py checks the reference itself, and that the probe's name table and the reference's are the same."""
import numpy as np
import pytest

import field_edge_ref as F

pytestmark = pytest.mark.gpu


def _mismatch(name, ops, got, want):
    bad = np.nonzero((got != want).any(axis=1))[0]
    return "%d of %d rows differ\n%s" % (len(bad), len(want), "\n".join(F.describe(name, ops, got, want, int(i)) for i in bad[:4]))


@pytest.mark.parametrize("name", [n for n in F.names() if n not in F.LIVE])
def test_primitive_word_for_word(hip, name):
    from ezkl_amd import backend as B
    ops, want, _ = F.case(name)
    got = B.field_probe(name, ops)
    assert got.shape == want.shape
    assert (got == want).all(), _mismatch(name, ops, got, want)
    field, prim = name.split(".")
    if prim == "mul_lazy":                                   # the butterflies rely on it: below 2p without a final subtraction
        assert all(F.from_words32(r) < 2 * F.MODS[field] for r in got.tolist())
    if field.endswith("29") and prim in ("normalize", "mul", "mul_cold", "sqr", "sqr_cold", "mul2add", "canonical") or prim.startswith("cond_sub"):
        assert (got[:, :8] <= F.M29).all()


@pytest.mark.parametrize("name", sorted(F.LIVE))
def test_product_leaves_live_registers_alone(hip, name):
    from ezkl_amd import backend as B
    ops, want, _ = F.case(name)
    got = B.field_probe(name, ops)
    w = ops[0].shape[1]
    assert (got[:, :w] == want[:, :w]).all(), "the product itself: " + _mismatch(name, ops, got[:, :w], want[:, :w])
    rows = slice(w, w + F.LIVE_ROWS * w)
    assert (got[:, rows] == want[:, rows]).all(), "operand rows held in vector registers across the product came back changed: " + _mismatch(name, ops, got[:, rows], want[:, rows])
    salt = slice(w + F.LIVE_ROWS * w, None)
    assert (got[:, salt] == want[:, salt]).all(), "words held in scalar registers across the product came back changed: " + _mismatch(name, ops, got[:, salt], want[:, salt])


def test_unknown_name_is_refused(hip):
    from ezkl_amd import backend as B, lib as L
    import ctypes as C
    buf = B.DeviceBuffer(64)
    arr = (C.c_void_p * 4)(buf.ptr, buf.ptr, None, None)
    for name in (b"fr.nothing", b"add", b"fr29.mul2add", b""):
        assert L.load().ezkl_hip_field_probe_dev(name, arr, C.c_void_p(buf.ptr), C.c_size_t(1), C.c_void_p(None)) == -3       # EZKL_ERR_INVALID
    buf.free()
