"""The host half of the SRS file check, without a device: ezkl_prover_srs_pairing_check on the golden k = 6 file with the random combination
made by the oracle's MSM, what it refuses to compute with, and the front doors of execute.check_srs and EZKL_SRS_CHECK."""
import ctypes as C

import numpy as np
import pytest

import srs_check_ref as CR
from conftest import rand_fr
from ezkl_amd import codecs, lib as L, native as NV
from oracle import binding as ob


@pytest.fixture(scope="module")
def combination(golden_srs):
    """(A, B, g2, s_g2): A = sum r_i g[i], B = sum r_i g[i + 1] over the 63 adjacent pairs, by the oracle's MSM"""
    srs = codecs.read_srs(golden_srs["buf"])
    r = rand_fr(np.random.default_rng(61), 63)
    g = np.ascontiguousarray(srs["g"])
    return ob.msm(r, g[:63].copy()), ob.msm(r, g[1:].copy()), srs["g2"], srs["s_g2"]


def test_pairing_accepts_the_golden_file_and_rejects_what_is_not_its_secret(combination):
    a, b, g2, s_g2 = combination
    assert CR.reason(a) == CR.reason(b) == (0, False)
    assert NV.srs_pairing_check(a, b, g2, s_g2) is True
    assert NV.srs_pairing_check(a, b, g2, g2) is False                     # s_g2 replaced by g2: the secret would be 1
    assert NV.srs_pairing_check(b, a, g2, s_g2) is False                   # A and B swapped: the secret would be 1 / s


def test_pairing_refuses_operands_outside_their_groups(combination):
    a, b, g2, s_g2 = combination
    off_twist = bytearray(s_g2)
    off_twist[40] ^= 1                                                      # one byte of x.c1
    with pytest.raises(NV.SrsOperandError, match="s_g2: point not on the twist"):
        NV.srs_pairing_check(a, b, g2, bytes(off_twist))
    with pytest.raises(NV.SrsOperandError, match="g2 is the identity"):
        NV.srs_pairing_check(a, b, bytes(128), s_g2)
    with pytest.raises(NV.SrsOperandError, match="s_g2 is the identity"):
        NV.srs_pairing_check(a, b, g2, bytes(128))
    big = bytearray(g2)
    big[0:32] = (CR.Q + 1).to_bytes(32, "little")
    with pytest.raises(NV.SrsOperandError, match="g2: coordinate not below the field modulus"):
        NV.srs_pairing_check(a, b, bytes(big), s_g2)
    for why, text in ((1, "x not below"), (2, "y not below"), (3, "a: point not on the curve")):
        with pytest.raises(NV.SrsOperandError, match=text):
            NV.srs_pairing_check(CR.bad_point(why), b, g2, s_g2)
    with pytest.raises(NV.SrsOperandError, match="b: point not on the curve"):
        NV.srs_pairing_check(a, CR.bad_point(3), g2, s_g2)
    assert NV.srs_pairing_check(a, b, g2, s_g2) is True                     # a good call clears the text of the failed ones
    assert NV.load().ezkl_prover_last_error() == b""


def test_pairing_refuses_a_twist_point_outside_the_order_r_subgroup(combination):
    """the twist's cofactor is not 1: a point of E'(Fq2) found by taking any x with a square right-hand side is on the twist and (with
    overwhelming probability) not of order r -- on-curve alone must not pass"""
    a, b, g2, s_g2 = combination
    Q = CR.Q
    def mul2(u, v): return ((u[0] * v[0] - u[1] * v[1]) % Q, (u[0] * v[1] + u[1] * v[0]) % Q)
    def pow2(u, e):
        acc = (1, 0)
        while e:
            if e & 1: acc = mul2(acc, u)
            u, e = mul2(u, u), e >> 1
        return acc
    xi_inv = pow2((9, 1), Q * Q - 2)
    bt = mul2((3, 0), xi_inv)                                               # 3 / (9 + u)
    x = (2, 1)
    while True:
        x3 = mul2(mul2(x, x), x)
        rhs = ((x3[0] + bt[0]) % Q, (x3[1] + bt[1]) % Q)
        if pow2(rhs, (Q * Q - 1) // 2) == (1, 0):
            break
        x = (x[0] + 1, x[1])
    # a square root in Fq2 (q^2 = 9 mod 16): Tonelli-Shanks over the 2-part of q^2 - 1
    s, t = 0, Q * Q - 1
    while t % 2 == 0: s, t = s + 1, t // 2
    z = (1, 1)
    while pow2(z, (Q * Q - 1) // 2) == (1, 0): z = (z[0] + 1, z[1])
    c, y, tt, m = pow2(z, t), pow2(rhs, (t + 1) // 2), pow2(rhs, t), s
    while tt != (1, 0):
        i, w = 0, tt
        while w != (1, 0): w, i = mul2(w, w), i + 1
        bb = c
        for _ in range(m - i - 1): bb = mul2(bb, bb)
        y, c, m = mul2(y, bb), mul2(bb, bb), i
        tt = mul2(tt, c)
    assert mul2(y, y) == rhs
    pt = b"".join((v * CR.MONT % Q).to_bytes(32, "little") for v in (x[0], x[1], y[0], y[1]))
    with pytest.raises(NV.SrsOperandError, match="s_g2: point not of order r"):
        NV.srs_pairing_check(a, b, g2, pt)


def test_both_identities_answer_ok_without_a_pairing(combination):
    _, _, g2, s_g2 = combination
    ident = np.zeros(8, np.uint64)
    assert NV.srs_pairing_check(ident, ident, g2, s_g2) is True
    assert NV.srs_pairing_check(ident, ident, g2, g2) is True              # no pairing is computed: whatever s_g2, a valid point suffices
    with pytest.raises(NV.SrsOperandError):                                  # ... but the G2 operands are still held to their group
        NV.srs_pairing_check(ident, ident, g2, bytes(128))


def test_one_identity_is_a_rejection(combination):
    a, _, g2, s_g2 = combination
    assert NV.srs_pairing_check(a, np.zeros(8, np.uint64), g2, s_g2) is False


@pytest.mark.skipif(L.load().ezkl_hip_device_count() > 0, reason="GPU present")
def test_check_srs_without_a_device_is_the_librarys_no_device_error():
    import os
    import ezkl_amd
    from conftest import GOLDEN
    from ezkl_amd import execute as X
    with pytest.raises(ezkl_amd.EzklHipError) as e:
        X.check_srs(os.path.join(GOLDEN, "kzg_k6.srs"))
    assert e.value.code == -1
    out = np.zeros(4, np.uint64)
    assert L.load().ezkl_hip_bases_check(None, C.c_size_t(0), C.c_size_t(0), out.ctypes.data_as(C.c_void_p)) == -3           # a null handle is refused before the device is asked for


def test_an_unknown_policy_is_refused_by_name(monkeypatch, tmp_path):
    from ezkl_amd import execute as X
    monkeypatch.setenv("EZKL_SRS_CHECK", "bogus")
    with pytest.raises(ValueError, match="EZKL_SRS_CHECK must be one of points, full, off; got 'bogus'"):
        X._srs_policy()
    import os
    from conftest import GOLDEN
    with pytest.raises(ValueError, match="EZKL_SRS_CHECK"):                  # and by the loaders, before any device work
        X.load_params_prover(os.path.join(GOLDEN, "kzg_k6.srs"), 6)
    for ok in ("points", "full", "off"):
        monkeypatch.setenv("EZKL_SRS_CHECK", ok)
        assert X._srs_policy() == ok
    monkeypatch.delenv("EZKL_SRS_CHECK")
    assert X._srs_policy() == "points"


def test_load_params_prover_of_a_same_size_file_needs_no_device():
    """a CPU caller's use of the loader stays free of device work under the default policy"""
    import os
    from conftest import GOLDEN
    from ezkl_amd import execute as X
    srs = X.load_params_prover(os.path.join(GOLDEN, "kzg_k6.srs"), 6)
    assert srs["k"] == 6 and srs["g"].shape == (64, 8)
