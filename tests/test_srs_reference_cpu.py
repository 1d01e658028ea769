"""The plain SRS reference of the GPU tests (tests/srs_ref.py) pinned on the CPU: the defining sum against the closed form, and the point
sets against the oracle's naive g_to_lagrange (one MSM of Lagrange-polynomial coefficients per point) -- ordinary and degenerate secrets."""
import numpy as np
import pytest
import srs_ref as SR
from oracle import binding as ob

ORDINARY = 0x1234567890abcdef1234567890abcdef % SR.R


def _secrets(k):
    return {"ordinary": ORDINARY, "zero": 0, "one": 1, "w3": pow(SR.omega(k), 3, SR.R)}


def test_root_and_generator_are_the_oracles():
    for k in (1, 4, 13, 28):
        assert (SR.fe(SR.omega(k)) == ob.omega(k)).all()
    assert pow(SR.ROOT, 1 << 27, SR.R) == SR.R - 1
    assert ob.g1_on_curve(SR.G)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6])
def test_closed_form_equals_the_defining_sum(k):
    for name, s in list(_secrets(k).items()) + [("minus_one", SR.R - 1), ("w_last", pow(SR.omega(k), (1 << k) - 1, SR.R))]:
        want = SR.lagrange_scalars_sum(s, k)
        assert SR.lagrange_scalars_closed(s, k) == want, name
        assert sum(want) % SR.R == 1, name                                         # the basis polynomials sum to 1


@pytest.mark.parametrize("k", [4, 6])
@pytest.mark.parametrize("name", ["ordinary", "zero", "one", "w3"])
def test_structured_set_equals_the_oracles_g_to_lagrange(k, name):
    s, n = _secrets(k)[name], 1 << k
    g, gl = SR.structured_set(s, k)
    assert g.shape == gl.shape == (n, 8)
    assert (g[0] == SR.G).all() and (g[1] == ob.g1_mul(SR.G, SR.fe(s))).all()
    assert gl.tobytes() == ob.g1_to_lagrange(g, k).tobytes()
    identities = int((~gl.any(axis=1)).sum())
    if name in ("one", "w3"):                                                       # a secret inside the domain: one G, n - 1 identities
        row = 0 if name == "one" else 3
        assert identities == n - 1 and (gl[row] == SR.G).all()
    else:
        assert identities == 0
    if name == "zero":                                                              # g = G, 0, 0, ...: every row is [1/n] G
        assert not g[1:].any() and (gl == gl[0]).all()
    assert SR.functional_check(g, gl, k, seed=k)


def test_helpers():
    p = ob.gen_bases(5, 1)[0]
    assert not ob.g1_add(p, SR.neg(p)).any() and not SR.neg(np.zeros(8, np.uint64)).any()
    sc = [0, 1, 2, SR.R - 1, 12345]
    got = SR.mul_many(p, sc)
    for row, c in zip(got, sc):
        assert (row == ob.g1_mul(p, SR.fe(c))).all()
    g, gl = SR.structured_set(ORDINARY, 4)
    bad = gl.copy(); bad[7] = g[3]
    assert not SR.functional_check(g, bad, 4, seed=1)                               # the check does see one wrong point


def test_gen_srs_refuses_a_secret_inside_the_domain_before_any_device_work(tmp_path):
    """backend.gen_srs / execute.gen_srs with s^n = 1: a ValueError that names the reason, raised before the first device call (so it is
    the same without a GPU) and before a file is written.  What a legal secret gives is compared on the device (tests/test_gpu_srs.py)."""
    from ezkl_amd import backend as B, execute as X
    for k in (3, 6):
        for s in (1, SR.R + 1, SR.R - 1, SR.omega(k), pow(SR.omega(k), (1 << k) - 1, SR.R)):
            with pytest.raises(ValueError, match="domain"):
                B.gen_srs(k, s)
            with pytest.raises(ValueError, match="domain"):
                X.gen_srs(str(tmp_path / "bad.srs"), k, secret=s)
    assert not (tmp_path / "bad.srs").exists()
