"""The G2 set check without a device: the entry point's name, wrapper and refusals, and -- in Python integers (tests/g2_check_ref.py) --
the endomorphism identity the kernel tests against the definition [r]P == O, with the psi constants read from the generated header."""
import ctypes as C
import inspect
import os
import re

import g2_check_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ezkl_hip_g2_check_dev"


def test_the_entry_point_is_declared_listed_once_exported_and_wrapped():
    from ezkl_amd import backend as B, lib as L
    header = open(os.path.join(ROOT, "include", "ezkl_hip.h")).read()
    assert re.search(r"int\s+%s\(const void\* points_dev, size_t n, uint64_t out\[4\], void\* stream\);" % NAME, header)
    assert header.index("ezkl_hip_msm_g2_points_dev(") < header.index(NAME + "(") < header.index("int ezkl_hip_msm_g1(")
    assert L.SYMBOLS.count(NAME) == 1
    assert hasattr(L.load(), NAME)
    assert list(inspect.signature(B.g2_check_points).parameters)[:1] == ["points"]
    assert inspect.signature(B.msm_g2_points).parameters["check"].default is False


def test_refusals_need_no_device_and_no_device_is_reported_not_computed():
    from ezkl_amd import lib as L
    f = getattr(L.load(), NAME)
    o, p = (C.c_uint64 * 4)(), C.c_void_p(0x1000)
    for args in ((None, 1, o), (p, 0, o), (p, 1, None), (C.c_void_p(0x1008), 1, o)):
        assert f(args[0], C.c_size_t(args[1]), args[2], None) == -3                               # EZKL_ERR_INVALID
    if L.load().ezkl_hip_device_count() > 0:                                                      # with a device the call would compute
        return
    assert f(p, C.c_size_t(1), o, None) == -1 and not any(o)                                      # EZKL_ERR_NO_DEVICE


def test_the_generated_psi_and_twist_constants_are_the_powers_of_xi():
    text = open(os.path.join(ROOT, "ezkl_amd", "csrc", "bn254_constants.h")).read()

    def const(name):
        c = []
        for half in ("C0", "C1"):
            limbs = re.search(r"#define BN32_FQ2_%s_%s_INIT \{(.*)\}" % (name, half), text).group(1).split(",")
            c.append(sum(int(l.strip().rstrip("u"), 16) << (32 * i) for i, l in enumerate(limbs)) * G.RINV % G.Q)
        return tuple(c)
    assert const("PSI_X") == G.f2_pow(G.XI, (G.Q - 1) // 3) == G.PSI_X
    assert const("PSI_Y") == G.f2_pow(G.XI, (G.Q - 1) // 2) == G.PSI_Y
    assert G.f2_mul(const("TWIST_B"), G.XI) == (3, 0)


def test_the_endomorphism_identity_agrees_with_the_order_on_32_good_and_32_bad_points():
    good, bad = G.good_points(32), G.twist_points(32)
    assert all(G.on_curve(p) for p in good + bad)
    assert all(G.in_subgroup(p) for p in good) and not any(G.in_subgroup(p) for p in bad)
    assert [G.endo_test(p) for p in good + bad] == [True] * 32 + [False] * 32
    assert G.endo_test(None) and G.endo_test(G.neg(good[4]))
