"""The SRS file check on the device: ezkl_hip_bases_check (g1_check_kernel, one lane per point) against the predicate restated in Python
integers (tests/srs_check_ref.py), the structural check of backend.check_srs against files tampered in ways only the structure can tell,
and the loaders of execute.py under the three EZKL_SRS_CHECK policies.  Tampered files are made here from the golden files, from
execute.gen_srs or from tests/srs_ref.py; point doublings are the oracle's additions."""
import json
import os

import numpy as np
import pytest

import fixture_k6 as FX
import srs_check_ref as CR
import srs_ref as SR
from conftest import GOLDEN, R, SEED
from oracle import binding as ob
from test_ezkl_circuit import FIXTURE_B, FIXTURE_W

pytestmark = pytest.mark.gpu

# The kernel's grid is one workgroup of 256 lanes per CU at the most: 2^16 lanes on the 256 CUs of an MI355X, so at 2^16 + 3 points
# three lanes walk the grid-stride loop a second time (indices 2^16 .. 2^16 + 2 are planted below for that).
BIG = (1 << 16) + 3
SIZES = [1, 63, 64, 65, 255, 256, 257, 1025, BIG]
S1 = 0x0123456789abcdef0fedcba987654321 % R
S2 = 0x1111111122222222333333334444444455555555 % R


@pytest.fixture(scope="module")
def clean():
    """n -> the first n points Bases.generate makes, downloaded once (read-only)"""
    from ezkl_amd import backend as B
    cache = {}
    def get(n):
        if n not in cache:
            b = B.Bases.generate(SEED + 3, n)
            cache[n] = b.download()
            cache[n].setflags(write=False)
            b.free()
        return cache[n]
    return get


def _check(pts, first=0, n=None):
    """upload, Bases.check, free -> (the device's answer, the reference's)"""
    from ezkl_amd import backend as B
    b = B.Bases(pts)
    try:
        return b.check(first, n), CR.check(pts, first, n)
    finally:
        b.free()


def _positions(n):
    """index 0 and n - 1, the wave edge 63 | 64, the workgroup edge 255 | 256, and past one grid where the set is that long"""
    return sorted({p for p in (0, n - 1, 63, 64, 255, 256, 1 << 16, (1 << 16) + 2) if p < n})


@pytest.mark.parametrize("n", SIZES)
def test_point_check_clean_and_one_bad_point_of_each_reason(hip, clean, n):
    got, want = _check(clean(n))
    assert got == want == dict(bad=0, first_bad=None, reason=0, identities=0)
    for pos in _positions(n):
        for why in (1, 2, 3):
            pts = clean(n).copy()
            pts[pos] = CR.bad_point(why, salt=pos)
            got, want = _check(pts)
            assert want == dict(bad=1, first_bad=pos, reason=why, identities=0)
            assert got == want, (n, pos, why)


@pytest.mark.parametrize("n", SIZES)
def test_point_check_two_bad_points_and_identities(hip, clean, n):
    pos = _positions(n)
    if len(pos) >= 2:
        for lo, hi in zip(pos, pos[1:]):                   # two reasons: the smaller index and ITS reason, whichever wave sees which
            for why_lo, why_hi in ((3, 1), (1, 3), (2, 3)):
                pts = clean(n).copy()
                pts[lo], pts[hi] = CR.bad_point(why_lo), CR.bad_point(why_hi)
                got, want = _check(pts)
                assert want == dict(bad=2, first_bad=lo, reason=why_lo, identities=0)
                assert got == want, (n, lo, hi)
    pts = clean(n).copy()
    pts[pos] = 0                                          # identities at the same positions: counted, not bad
    got, want = _check(pts)
    assert want == dict(bad=0, first_bad=None, reason=0, identities=len(pos))
    assert got == want
    if n > 2:                                             # ... and next to a bad point
        pts[n // 2] = CR.bad_point(2)
        got, want = _check(pts)
        assert got == want and got["bad"] == 1 and got["first_bad"] == n // 2


def test_point_check_all_points_bad(hip):
    n = 257
    pts = np.stack([CR.bad_point(1 + i % 3, salt=i) for i in range(n)])
    got, want = _check(pts)
    assert want == dict(bad=n, first_bad=0, reason=1, identities=0)
    assert got == want
    got, want = _check(pts, 1, n - 1)
    assert got == want == dict(bad=n - 1, first_bad=1, reason=2, identities=0)


@pytest.mark.parametrize("first,count", [(5, 100), (70, 130), (1, 255), (63, 2), (64, 193), (256, 1), (300, 700)])
def test_point_check_sub_ranges(hip, clean, first, count):
    """ranges that begin and end inside a wave: a bad point on either side of the range is not reported, one inside is, by its index
    in the SET"""
    pts = clean(1025).copy()
    pts[first - 1], pts[first + count] = CR.bad_point(3), CR.bad_point(1)
    got, want = _check(pts, first, count)
    assert got == want == dict(bad=0, first_bad=None, reason=0, identities=0)
    inside = first + count - 1
    pts[inside] = CR.bad_point(2)
    pts[first - 1] = 0                                     # (and an identity outside is not counted)
    got, want = _check(pts, first, count)
    assert got == want == dict(bad=1, first_bad=inside, reason=2, identities=0)


def test_point_check_empty_range_and_range_past_the_end(hip, clean):
    import ezkl_amd
    from ezkl_amd import backend as B
    pts = clean(65).copy()
    pts[3] = CR.bad_point(3)
    b = B.Bases(pts)
    try:
        for first in (0, 3, 65):
            assert b.check(first, 0) == dict(bad=0, first_bad=None, reason=0, identities=0)
        for first, count in ((0, 66), (65, 1), (66, 0), (1, (1 << 64) - 1)):
            with pytest.raises(ezkl_amd.EzklHipError) as e:
                b.check(first, count)
            assert e.value.code == -3
        assert b.check() == dict(bad=1, first_bad=3, reason=3, identities=0)
    finally:
        b.free()


# ------------------------------------------------------------------ the structural check
def _file(name):
    from ezkl_amd import codecs
    srs = codecs.read_srs(open(os.path.join(GOLDEN, name), "rb").read())
    return dict(srs, g=srs["g"].copy(), g_lagrange=srs["g_lagrange"].copy())


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    """(k, secret) -> the parsed file execute.gen_srs writes (made once)"""
    from ezkl_amd import codecs, execute as X
    cache, d = {}, tmp_path_factory.mktemp("srs")
    def get(k, s=S1):
        if (k, s) not in cache:
            path = str(d / ("kzg_%d_%x.srs" % (k, s & 0xffff)))
            X.gen_srs(path, k, secret=s)
            srs = codecs.read_srs(open(path, "rb").read())
            cache[(k, s)] = dict(srs, path=path)
        srs = cache[(k, s)]
        return dict(srs, g=srs["g"].copy(), g_lagrange=srs["g_lagrange"].copy())
    return get


@pytest.mark.parametrize("name", ["kzg_k1_public.srs", "kzg_k6.srs"])
def test_structure_of_the_golden_files(hip, name):
    from ezkl_amd import backend as B
    srs = _file(name)
    for seed in (1, 2, 3):
        rep = B.check_srs(srs, seed=seed)
        assert rep["ok"] and rep["reason"] is None and rep["powers"] is rep["lagrange"] is rep["g2"] is True, rep
        assert rep["k"] == srs["k"] and rep["key"] == B.srs_check_key(seed) and len(rep["key"]) == 32
        assert rep["points"] == {s: dict(bad=0, first_bad=None, reason=0, identities=0) for s in ("g", "g_lagrange")}
    assert B.check_srs(srs)["ok"]                          # OS entropy
    rep = B.check_srs(srs, structure=False)
    assert rep["ok"] and rep["powers"] is rep["lagrange"] is rep["g2"] is None


@pytest.mark.parametrize("k", [0, 10])
def test_structure_of_generated_files(hip, made, k):
    """k = 0: one point, no adjacent pair, a one-point Lagrange check; k = 10: 1024 points"""
    from ezkl_amd import backend as B, execute as X
    rep = B.check_srs(made(k), seed=5)
    assert rep["ok"] and rep["powers"] is rep["lagrange"] is rep["g2"] is True, rep
    assert X.check_srs(made(k)["path"], seed=5)["ok"]


@pytest.mark.parametrize("which", ["g", "g_lagrange"])
def test_every_index_takes_part_in_the_structural_check(hip, made, which):
    """k = 4: for every index, the point replaced by 2 x itself -- on the curve, so only the structure can tell.  A g tamper fails the
    powers check (index n - 1 is only ever a g[i + 1], index 0 only ever a g[i]); a g_lagrange tamper fails the Lagrange check alone."""
    from ezkl_amd import backend as B
    for i in range(16):
        srs = made(4)
        srs[which][i] = ob.g1_add(srs[which][i], srs[which][i])
        assert CR.reason(srs[which][i]) == (0, False)
        rep = B.check_srs(srs, seed=100 + i)
        assert not rep["ok"] and rep["points"][which]["bad"] == 0, (which, i, rep)
        if which == "g":
            assert rep["powers"] is False and rep["reason"] == "g: not consecutive powers of one secret", (i, rep)
        else:
            assert rep["powers"] is True and rep["lagrange"] is False and rep["reason"] == "g_lagrange is not the Lagrange basis of g", (i, rep)


def test_structure_rejects_swaps_and_parts_of_another_secret(hip, made):
    from ezkl_amd import backend as B
    srs = made(6)
    srs["g"][[10, 11]] = srs["g"][[11, 10]]
    rep = B.check_srs(srs, seed=7)
    assert not rep["ok"] and rep["powers"] is False
    other = made(6, S2)
    rep = B.check_srs(dict(made(6), g_lagrange=other["g_lagrange"]), seed=7)
    assert not rep["ok"] and rep["powers"] is True and rep["lagrange"] is False and rep["reason"] == "g_lagrange is not the Lagrange basis of g"
    rep = B.check_srs(dict(made(6), s_g2=other["s_g2"]), seed=7)
    assert not rep["ok"] and rep["g2"] is True and rep["powers"] is False and rep["lagrange"] is True
    twisted = bytearray(made(6)["s_g2"])
    twisted[3] ^= 0x10
    rep = B.check_srs(dict(made(6), s_g2=bytes(twisted)), seed=7)
    assert not rep["ok"] and rep["g2"] is False and "s_g2" in rep["reason"]


@pytest.mark.parametrize("secret", [0, 1])
def test_degenerate_sets_pass_the_point_check_and_fail_the_structure(hip, made, secret):
    """secret 0: g = (G, O, O, ...); secret 1: g_lagrange = (G, O, O, ...) -- 63 identities either way"""
    from ezkl_amd import backend as B, native as NV
    g, gl = SR.structured_set(secret, 6)
    srs = dict(k=6, g=g, g_lagrange=gl, g2=NV.g2_mul_generator(1), s_g2=made(6)["s_g2"])
    rep = B.check_srs(srs, structure=False)
    assert rep["ok"] and sum(rep["points"][s]["identities"] for s in ("g", "g_lagrange")) == 63 and rep["points"]["g"]["bad"] == 0
    rep = B.check_srs(srs, seed=1)
    assert not rep["ok"] and rep["reason"] == "degenerate set: 63 identities" and rep["powers"] is None


def test_the_combination_is_the_oracles_msm_of_the_same_scalars(hip):
    from ezkl_amd import backend as B
    srs = _file("kzg_k6.srs")
    key = B.srs_check_key(11)
    assert key == B.srs_check_key(11) != B.srs_check_key(12)
    r = B.DeviceBuffer(32 * 63)
    bg = B.Bases(srs["g"])
    try:
        B.chacha20_fr(key, 0, r.ptr, 63)
        scalars = r.to_numpy(shape=(63, 4))
        a, b = B.srs_power_combination(bg, key)
    finally:
        r.free(); bg.free()
    assert a.tobytes() == ob.msm(scalars, srs["g"][:63].copy()).tobytes()
    assert b.tobytes() == ob.msm(scalars, srs["g"][1:].copy()).tobytes()


# ------------------------------------------------------------------ the loaders
@pytest.fixture()
def circuit_file(tmp_path):
    st = json.load(open(os.path.join(FX.G, "settings_k6.json")))
    assert st["run_args"]["logrows"] == 6
    compiled = tmp_path / "model.compiled.json"
    compiled.write_text(json.dumps({"model": "mlp", "run_args": st["run_args"], "weights": [FIXTURE_W], "biases": [FIXTURE_B],
                                    "total_assignments": st["total_assignments"]}))
    return str(compiled)


def _write(tmp_path, name, srs):
    from ezkl_amd import codecs
    path = tmp_path / name
    path.write_bytes(codecs.write_srs(srs))
    return str(path)


def test_loaders_refuse_a_bad_point_they_would_use(hip, tmp_path, circuit_file, monkeypatch):
    from ezkl_amd import execute as X
    monkeypatch.delenv("EZKL_SRS_CHECK", raising=False)
    srs = _file("kzg_k6.srs")
    srs["g"][37] = CR.bad_point(3)
    bad = _write(tmp_path, "bad.srs", srs)
    vk, pk = str(tmp_path / "vk.key"), str(tmp_path / "pk.key")
    with pytest.raises(X.SrsError, match=r"g\[37\]: point not on the curve") as e:
        X.setup(circuit_file, bad, vk, pk)
    assert e.value.report["points"]["g"] == dict(bad=1, first_bad=37, reason=3, identities=0) and not os.path.exists(pk)
    g = lambda name: os.path.join(FX.G, name)
    with pytest.raises(X.SrsError, match=r"g\[37\]: point not on the curve"):
        X.Prover(g("model_k6.compiled"), g("pk_k6.key"), bad, recommit=True)
    with pytest.raises(X.SrsError, match=r"g\[37\]: point not on the curve"):
        X.check_srs(bad)
    srs = _file("kzg_k6.srs")
    srs["g_lagrange"][63] = CR.bad_point(2)
    with pytest.raises(X.SrsError, match=r"g_lagrange\[63\]: y coordinate not below the field modulus"):
        X.Prover(g("model_k6.compiled"), g("pk_k6.key"), _write(tmp_path, "bad_gl.srs", srs), recommit=True)
    monkeypatch.setenv("EZKL_SRS_CHECK", "off")                       # the caller's choice: nothing is checked
    X.setup(circuit_file, bad, vk, pk)
    assert os.path.getsize(pk) > 0
    X.Prover(g("model_k6.compiled"), g("pk_k6.key"), bad, recommit=True).close()


def test_a_bad_point_beyond_the_circuit_is_not_the_loaders_business(hip, tmp_path, circuit_file, made, monkeypatch):
    """a k = 7 file downsized to the k = 6 circuit: only g[:64] is used, and only that is checked under the default policy"""
    from ezkl_amd import execute as X
    monkeypatch.delenv("EZKL_SRS_CHECK", raising=False)
    srs = made(7)
    keys = []
    for name, tamper in (("clean7.srs", False), ("bad7.srs", True)):
        if tamper:
            srs["g"][100] = CR.bad_point(3)
            srs["g_lagrange"][5] = CR.bad_point(1)         # the file's own Lagrange basis is not used either
        pk = tmp_path / (name + ".pk")
        X.setup(circuit_file, _write(tmp_path, name, srs), str(tmp_path / "vk.key"), str(pk))
        keys.append(pk.read_bytes())
    assert keys[0] == keys[1]
    with pytest.raises(X.SrsError, match=r"g\[100\]: point not on the curve"):
        X.check_srs(str(tmp_path / "bad7.srs"))           # the whole file, whatever circuit it serves
    srs["g"][64 - 1] = CR.bad_point(3)                     # the last point that IS used
    with pytest.raises(X.SrsError, match=r"g\[63\]: point not on the curve"):
        X.setup(circuit_file, _write(tmp_path, "bad7b.srs", srs), str(tmp_path / "vk.key"), str(tmp_path / "pk.key"))


def test_full_policy_refuses_a_wrong_lagrange_basis(hip, tmp_path, circuit_file, monkeypatch):
    from ezkl_amd import execute as X
    srs = _file("kzg_k6.srs")
    srs["g_lagrange"][20] = ob.g1_add(srs["g_lagrange"][20], srs["g_lagrange"][20])
    path = _write(tmp_path, "doubled.srs", srs)
    monkeypatch.setenv("EZKL_SRS_CHECK", "full")
    with pytest.raises(X.SrsError, match="g_lagrange is not the Lagrange basis of g") as e:
        X.setup(circuit_file, path, str(tmp_path / "vk.key"), str(tmp_path / "pk.key"))
    assert e.value.report["lagrange"] is False and e.value.report["powers"] is True
    monkeypatch.setenv("EZKL_SRS_CHECK", "points")                    # on the curve: the point check cannot tell
    X.setup(circuit_file, path, str(tmp_path / "vk.key"), str(tmp_path / "pk.key"))


def test_the_golden_file_proves_to_the_same_bytes_under_every_policy(hip, tmp_path, circuit_file, monkeypatch):
    from ezkl_amd import execute as X
    srs, wit = os.path.join(FX.G, "kzg_k6.srs"), os.path.join(FX.G, "witness_k6.json")
    out = {}
    for policy in ("points", "full", "off"):
        monkeypatch.setenv("EZKL_SRS_CHECK", policy)
        vk, pk, proof_path = (str(tmp_path / (policy + ext)) for ext in (".vk", ".pk", ".proof.json"))
        X.setup(circuit_file, srs, vk, pk)
        proof = X.prove(wit, circuit_file, pk, proof_path, srs, X.CheckMode.SAFE, seed=42)
        assert X.verify(proof_path, circuit_file, vk, srs)
        out[policy] = (open(pk, "rb").read(), proof)
    assert out["points"] == out["full"] == out["off"]
