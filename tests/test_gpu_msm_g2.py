"""GPU parity of the G2 bucket MSM (backend.msm_g2_points: ezkl_hip_msm_g2_points_dev, csrc/g2.hip) with the oracle's G2 arithmetic in
Python integers (oracle/pairing.py: g2_mul).  The points are small multiples k_j G of the generator, as the golden k = 6 SRS's tail holds
(g2 = G), so the expected sum is ONE oracle scalar multiplication, [sum_i s_i k_i mod r] G, and every case runs in seconds."""
import ctypes as C

import numpy as np
import pytest

import srs_ref as SR
from conftest import R, fe_to_int, rand_fr
from test_gpu_srs import G2, _g2_enc, _g2_dec

pytestmark = pytest.mark.gpu
NP = 13            # multiples 1 .. 12 of G, their negatives, and the identity record at index 0


@pytest.fixture(scope="module")
def table():
    """ks[j], enc[j]: the discrete logs (mod r) and the encoded records of 0, +-1 G .. +-12 G -- computed once, shared, never changed"""
    from oracle import pairing as E
    ks, enc = [0], [_g2_enc(None)]
    for k in range(1, NP):
        p = E.g2_mul(G2, k)
        ks += [k, R - k]
        enc += [_g2_enc(p), _g2_enc((p[0], E.f2_neg(p[1])))]
    return ks, np.stack(enc)


def _want(ks, idx, sc):
    from oracle import pairing as E
    return E.g2_mul(G2, sum(s * ks[i] for s, i in zip(sc, idx)) % R)


def _run(hip, enc, idx, sc):
    from ezkl_amd import backend as B
    dp, ds = B.DeviceBuffer.from_numpy(np.ascontiguousarray(enc[idx])), B.DeviceBuffer.from_numpy(SR.fes(sc))
    try:
        return _g2_dec(B.msm_g2_points(dp, ds))
    finally:
        dp.free(); ds.free()


def _sizes():
    from ezkl_amd import backend as B
    return sorted({1, 2, 63, 64, 65, 255, 257, B.MSM_G2_SORT_TILE + 1, B.MSM_G2_CROSSOVER + 1})


@pytest.mark.parametrize("kind", ["uniform", "zero", "one", "r-1", "equal", "last"])
@pytest.mark.parametrize("n", _sizes())
def test_sizes_and_scalar_kinds_match_the_oracle(hip, table, n, kind):
    """wave, workgroup, sort-tile and crossover edges x scalar shapes: full-width digits; nothing; one digit; every digit negative; one bucket
    per window taking all n pairs (the long-run kernel once n outgrows long_run); one pair in all"""
    ks, enc = table
    rng = np.random.default_rng(n)
    idx = rng.integers(1, len(ks), n)                                     # no identity records here: see the pattern test
    sc = {"uniform": lambda: [fe_to_int(v) for v in rand_fr(rng, n)], "zero": lambda: [0] * n, "one": lambda: [1] * n, "r-1": lambda: [R - 1] * n,
          "equal": lambda: [fe_to_int(rand_fr(rng, 1)[0])] * n, "last": lambda: [0] * (n - 1) + [(1 << 253) - 1]}[kind]()
    want = _want(ks, idx, sc)
    assert kind != "zero" or want is None
    assert _run(hip, enc, idx, sc) == want


@pytest.mark.parametrize("pattern", ["identities", "all-equal", "cancel", "cancel-but-one"])
def test_point_patterns_at_65_points_match_the_oracle(hip, table, pattern):
    """identity records at the first, a middle and the last index; one point throughout (the first addition into a bucket's XYZZ sum P is
    P + P); P, -P alternating under equal scalars (every bucket cancels: (0, 0)); the same with one survivor"""
    ks, enc = table
    n, rng = 65, np.random.default_rng(65)
    sc = [fe_to_int(v) for v in rand_fr(rng, n)]
    idx = rng.integers(1, len(ks), n)
    if pattern == "identities":
        idx[[0, 31, 64]] = 0
    elif pattern == "all-equal":
        idx[:], sc = 5, [sc[0]] * n
    else:
        idx = np.array([9 + (i & 1) for i in range(n)])                   # 5 G, -5 G, 5 G, ...
        sc = [sc[0]] * n
        if pattern == "cancel":
            idx[64] = 0                                                   # 32 pairs and an identity record
    want = _want(ks, idx, sc)
    assert (want is None) == (pattern == "cancel")
    assert _run(hip, enc, idx, sc) == want


def test_host_form_is_the_same_on_both_sides_of_the_crossover(hip, table):
    """ezkl_hip_msm_g2 one point below the crossover (the double-and-add kernel) and one above (upload + the bucket chain), over the same
    three live rows at the end and zero scalars before them (which the double-and-add kernel passes quickly): equal bytes, equal to the oracle"""
    from ezkl_amd import backend as B
    ks, enc = table
    n = B.MSM_G2_CROSSOVER + 1
    rng = np.random.default_rng(7)
    idx, sc = rng.integers(0, len(ks), n), [0] * (n - 3) + [fe_to_int(v) for v in rand_fr(rng, 3)]
    below, above = B.msm_g2(enc[idx[2:]], SR.fes(sc[2:])), B.msm_g2(enc[idx], SR.fes(sc))
    want = _want(ks, idx, sc)
    assert want is not None and _g2_dec(below) == want == _g2_dec(above)
    assert below.tobytes() == above.tobytes()


def test_refusals(hip):
    from ezkl_amd import backend as B, lib as L
    f, o = L.load().ezkl_hip_msm_g2_points_dev, (C.c_uint64 * 16)()
    d = B.DeviceBuffer(128)
    try:
        p = C.c_void_p(d.ptr)
        assert f(p, p, C.c_size_t(0), o, None) == f(None, p, C.c_size_t(1), o, None) == f(p, None, C.c_size_t(1), o, None) == -3
        assert f(p, p, C.c_size_t(1), None, None) == -3
    finally:
        d.free()
