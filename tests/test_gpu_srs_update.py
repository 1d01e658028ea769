"""The SRS update on the device: g1_mul_rows_kernel (Bases.mul_scalars, out[i] = scalars[i] * points[i]) against the oracle's
double-and-add over every row; backend.update_srs against its exact oracle -- updating gen_srs(k, s) with t gives, byte for byte, the
file gen_srs(k, s t mod r) writes, canonical affine points being unique --; verify_srs_update on real and on tampered updates; and the
two front doors of execute.py on files, with a proof under the updated SRS.  Every comparison is an equality."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import fixture_k6 as FX
import srs_ref as SR
from conftest import Q, R, SEED, fe_to_int, rand_fr
from oracle import binding as ob

pytestmark = pytest.mark.gpu

ALL_ONES = lambda bits, shift: ((1 << bits) - 1) << shift
# the edges of the double-and-add over the canonical bits 253 .. 0: nothing to add, one addition and no doubling, the largest canonical
# value (the negated point), bit 253 alone and with company, and a run of sixteen ones across every boundary of the 32-bit limbs the
# loop reads its bits from (bits 24 .. 39, 56 .. 71, ...: the 64-bit boundaries are among them), one run across three limbs
EDGES = [0, 1, R - 1, 1 << 253, (1 << 253) + 1, R - 2, (1 << 253) - 1, 2, ALL_ONES(70, 29)] + [ALL_ONES(16, 32 * j - 8) for j in range(1, 8)]
assert all(0 <= e < R for e in EDGES) and len(set(EDGES)) == len(EDGES) == 16
EDGE_ROWS = (0, 63, 64, 255, 256)


def _bad_rows(got, want):
    return np.flatnonzero((np.asarray(got) != np.asarray(want)).any(axis=1)).tolist()


def _scalar_column(n, seed, turn=0):
    """uniform values of Fr with EDGES on rows 0, 63, 64, 255, 256 and n - 1 and, where the column has room, all of them spread in
    between; `turn` rotates which edge lands on which row -> canonical integers"""
    col = [fe_to_int(v) for v in rand_fr(np.random.default_rng(seed), n)]
    rows = list(dict.fromkeys([r for r in EDGE_ROWS if r < n] + [n - 1]))
    if n > 2 * len(EDGES):
        rows += [int(r) for r in np.linspace(1, n - 2, 2 * len(EDGES)).round() if int(r) not in rows]
    for j, r in enumerate(rows):
        col[r] = EDGES[(j + turn) % len(EDGES)]
    assert n <= 2 * len(EDGES) or set(EDGES) <= set(col)
    return col


def _mul_rows(points, scalars):
    """[[scalars[i]] points[i]] by the oracle's double-and-add, one call per row; an identity row stays the all-zero record"""
    sc = SR.fes(scalars)
    out = np.zeros((len(scalars), 8), np.uint64)

    def work(lo):
        for i in range(lo, min(lo + 64, len(scalars))):
            if points[i].any():
                out[i] = ob.g1_mul(points[i], sc[i])
    with ThreadPoolExecutor(max(1, min(16, ob.effective_cpus()))) as ex:
        list(ex.map(work, range(0, len(scalars), 64)))
    return out


@pytest.fixture(scope="module")
def points():
    """1025 generated points (read-only); [:n] is the set of a smaller case"""
    p = ob.gen_bases(SEED + 21, 1025).copy()
    p.setflags(write=False)
    return p


def _run(B, bases, col, first=0, n=None):
    dev = B.DeviceBuffer.from_numpy(SR.fes(col))
    try:
        out = bases.mul_scalars(dev.ptr, first, n)
        try:
            assert out.n == len(col)
            return out.download()
        finally:
            out.free()
    finally:
        dev.free()


@pytest.mark.parametrize("identities", [False, True], ids=["points", "identities_at_the_edges"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
def test_mul_scalars_matches_double_and_add_on_every_row(hip, points, n, identities):
    """EVERY row against oracle.binding.g1_mul at the sizes from_scalars is tested at (one lane, one workgroup of 256 less one, exactly
    one, one more, past four), the scalar edges on the rows at the wave and workgroup edges and on the last row, uniform scalars
    elsewhere: neighbouring lanes of a wave hold unrelated scalars.  With identities planted on either side of the wave edge 63 | 64 and
    of the workgroup edge 255 | 256 those rows come out as the all-zero record.  The same handle is then run with other scalars (the
    edges moved on by five): that result is right as well, differs from the first, and the handle's own points are unchanged."""
    from ezkl_amd import backend as B
    pts = points[:n].copy()
    if identities:
        pts[[r for r in (63, 64, 255, 256) if r < n]] = 0
        if n == 1:
            pts[0] = 0
    bases = B.Bases(pts)
    try:
        cols = [_scalar_column(n, 100 + n, turn) for turn in (0, 5)]
        if n == 1:
            cols = [[e] for e in EDGES]                           # one lane: every edge in turn
        got = [_run(B, bases, col) for col in cols]
        assert bases.download().tobytes() == pts.tobytes()
    finally:
        bases.free()
    for col, out in zip(cols, got):
        assert out.shape == (n, 8)
        bad = _bad_rows(out, _mul_rows(pts, col))
        assert not bad, "rows %s differ; their scalars: %s" % (bad, [hex(col[r]) for r in bad[:8]])
        assert not out[[r for r in range(n) if col[r] == 0 or not pts[r].any()]].any()
    if not identities:
        assert got[0].tobytes() != got[1].tobytes()
        one = [r for r in range(n) if cols[0][r] == 1]
        assert (got[0][one] == pts[one]).all()                    # scalar 1: the point itself
        neg = [r for r in range(n) if cols[0][r] == R - 1]
        assert (got[0][neg] == np.stack([SR.neg(pts[r]) for r in neg])).all() if neg else True      # r - 1: the negated point


def test_mul_scalars_on_a_sub_range(hip, points):
    """first = 3, n = 250 on a 257-point set: row i of the result is scalar i times point 3 + i.  Identities on the first and the last
    point of the range and inside it; the points just outside the range (2 and 253, an identity and a record that is no point at all)
    are never read into the result."""
    from ezkl_amd import backend as B
    first, n = 3, 250
    pts = points[:257].copy()
    pts[[2, first, 64, first + n - 1]] = 0
    pts[first + n] = np.uint64(0xffffffffffffffff)
    col = _scalar_column(n, 7)
    bases = B.Bases(pts)
    try:
        got = _run(B, bases, col, first, n)
        whole = _run(B, bases, [1] * 252, 0, 252)                 # another range of the same handle, the neutral scalar
    finally:
        bases.free()
    assert got.shape == (n, 8)
    assert not _bad_rows(got, _mul_rows(pts[first:first + n], col))
    assert not got[[0, 64 - first, n - 1]].any()
    assert whole.tobytes() == pts[:252].tobytes()


def test_mul_scalars_refuses_a_range_past_the_set_and_an_empty_one(hip, points):
    import ezkl_amd
    from ezkl_amd import backend as B
    bases = B.Bases(points[:65].copy())
    dev = B.DeviceBuffer.from_numpy(SR.fes([1] * 65))
    try:
        for first, n in ((0, 66), (65, 1), (66, 0), (1, 65), (1, (1 << 64) - 1), (0, 0), (65, 0)):
            with pytest.raises(ezkl_amd.EzklHipError) as e:
                bases.mul_scalars(dev.ptr, first, n)
            assert e.value.code == -3, (first, n)
        last = bases.mul_scalars(dev.ptr, 64, 1)                  # the last point alone is a legal range
        assert last.download().tobytes() == points[64:65].tobytes()
        last.free()
    finally:
        dev.free(); bases.free()


# ------------------------------------------------------------------ update_srs against gen_srs
S_SMALL = 5
S_WIDE = 0x2b3c4d5e6f708192a3b4c5d6e7f8091a2b3c4d5e6f708192a3b4c5d6e7f8091a          # 254 bits, below r
T_WIDE = 0x1f2e3d4c5b6a79880796a5b4c3d2e1f00f1e2d3c4b5a69788796a5b4c3d2e1f0
assert S_WIDE.bit_length() == 254 and S_WIDE < R and 1 < T_WIDE < R


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    """(k, secret) -> the parsed file execute.gen_srs writes, with its path and bytes (made once; read-only)"""
    from ezkl_amd import codecs, execute as X
    cache, d = {}, tmp_path_factory.mktemp("srs_update")
    def get(k, s):
        if (k, s) not in cache:
            path = str(d / ("kzg_%d_%d.srs" % (k, len(cache))))
            X.gen_srs(path, k, secret=s)
            raw = open(path, "rb").read()
            cache[(k, s)] = dict(codecs.read_srs(raw), path=path, raw=raw)
        return cache[(k, s)]
    return get


@pytest.mark.parametrize("t", [7, R - 2, T_WIDE], ids=["t7", "t_r_minus_2", "t_wide"])
@pytest.mark.parametrize("s", [S_SMALL, S_WIDE], ids=["s5", "s_wide"])
@pytest.mark.parametrize("k", [4, 8, 9, 10])
def test_update_of_a_generated_file_is_the_file_generated_from_the_product(hip, made, k, s, t):
    from ezkl_amd import backend as B, codecs
    st = s * t % R
    assert pow(st, 1 << k, R) != 1 and pow(s, 1 << k, R) != 1          # gen_srs stays inside its domain on both sides
    want = made(k, st)
    new, proof = B.update_srs(made(k, s), t)
    assert set(proof) == {"t_g2"} and len(proof["t_g2"]) == 128
    assert new["k"] == k and new["g2"] == want["g2"]
    assert not _bad_rows(new["g"], want["g"])
    assert not _bad_rows(new["g_lagrange"], want["g_lagrange"])
    assert new["s_g2"] == want["s_g2"]
    assert codecs.write_srs(new) == want["raw"]
    assert proof["t_g2"] == made(4, t)["s_g2"]                         # [t] g2 is the s_g2 of a file whose secret is t


def test_update_by_one_returns_the_files_bytes_and_two_updates_compose(hip, made):
    from ezkl_amd import backend as B, codecs
    k, s, t1, t2 = 8, S_WIDE, 11, T_WIDE
    old = made(k, s)
    same, proof = B.update_srs(old, 1)
    assert codecs.write_srs(same) == old["raw"] and proof["t_g2"] == old["g2"]
    step1, _ = B.update_srs(old, t1)
    step2, _ = B.update_srs(step1, t2)
    both, _ = B.update_srs(old, t1 * t2 % R)
    assert codecs.write_srs(step2) == codecs.write_srs(both) != old["raw"]
    assert pow(s * t1 * t2 % R, 1 << k, R) != 1 and codecs.write_srs(both) == made(k, s * t1 * t2 % R)["raw"]


# ------------------------------------------------------------------ verify_srs_update
@pytest.fixture(scope="module")
def update6(hip, made):
    """a real update at k = 6: (old, new, proof, t)"""
    from ezkl_amd import backend as B
    t = T_WIDE
    new, proof = B.update_srs(made(6, S_WIDE), t)
    return made(6, S_WIDE), new, proof, t


def test_verify_accepts_a_real_update(update6):
    from ezkl_amd import backend as B
    old, new, proof, _ = update6
    rep = B.verify_srs_update(old, new, proof, seed=3)
    assert rep["ok"] and rep["reason"] is None and rep["k"] == 6 and rep["t_g2"] is True and rep["link"] is True
    assert rep["old"]["ok"] and rep["new"]["ok"] and rep["new"]["lagrange"] is True and rep["new"]["powers"] is True
    assert B.verify_srs_update(old, new, proof)["ok"]                  # OS entropy


def test_verify_rejects_each_tampering_at_its_step(update6, made):
    from ezkl_amd import backend as B
    old, new, proof, t = update6
    reject = lambda o, n, p: B.verify_srs_update(o, n, p, seed=4)
    # a new file made with another secret, against the proof of t: both files are sound, the link fails
    other, other_proof = B.update_srs(old, t + 1)
    rep = reject(old, other, proof)
    assert not rep["ok"] and rep["reason"].startswith("link:") and rep["link"] is False and rep["old"]["ok"] and rep["new"]["ok"]
    assert reject(old, other, other_proof)["ok"]
    # old and new swapped: t^2 != 1
    rep = reject(new, old, proof)
    assert not rep["ok"] and rep["reason"].startswith("link:")
    # two entries of the new Lagrange basis exchanged: valid points both, only the structure tells
    gl = new["g_lagrange"].copy()
    gl[[5, 40]] = gl[[40, 5]]
    rep = reject(old, dict(new, g_lagrange=gl), proof)
    assert not rep["ok"] and rep["reason"] == "new: g_lagrange is not the Lagrange basis of g" and rep["new"]["lagrange"] is False and rep["link"] is None
    # ... and of the old one
    gl = old["g_lagrange"].copy()
    gl[[0, 63]] = gl[[63, 0]]
    rep = reject(dict(old, g_lagrange=gl), new, proof)
    assert not rep["ok"] and rep["reason"] == "old: g_lagrange is not the Lagrange basis of g" and rep["new"] is None
    # s_g2' left as it was: g' is a sequence of powers, but not of that secret
    rep = reject(old, dict(new, s_g2=old["s_g2"]), proof)
    assert not rep["ok"] and rep["reason"] == "new: g: not consecutive powers of one secret"
    # t_g2: the identity, a coordinate that is not canonical, a wrong length
    rep = reject(old, new, dict(t_g2=bytes(128)))
    assert not rep["ok"] and rep["reason"].startswith("t_g2 is the identity") and rep["t_g2"] is False and rep["link"] is None
    x0 = int.from_bytes(proof["t_g2"][:32], "little")
    assert x0 + Q < 1 << 256
    rep = reject(old, new, dict(t_g2=(x0 + Q).to_bytes(32, "little") + proof["t_g2"][32:]))
    assert not rep["ok"] and rep["reason"].startswith("t_g2: coordinate not below the field modulus") and rep["t_g2"] is False
    rep = reject(old, new, dict(t_g2=proof["t_g2"][:64]))
    assert not rep["ok"] and rep["reason"].startswith("t_g2:")
    # files of different k; another g2; another first point
    rep = reject(old, made(4, S_SMALL), proof)
    assert not rep["ok"] and rep["reason"] == "k: the old file has k = 6, the new one k = 4" and rep["old"] is None
    rep = reject(old, dict(new, g2=new["s_g2"]), proof)
    assert not rep["ok"] and rep["reason"].startswith("g2:")
    g = new["g"].copy()
    g[0] = g[1]
    rep = reject(old, dict(new, g=g), proof)
    assert not rep["ok"] and rep["reason"].startswith("g[0]:")


def test_a_secret_that_lands_in_the_domain_is_reported_as_the_degenerate_set_it_makes(hip, made):
    """t = w / s: (s t)^n = 1.  update_srs cannot know (it never sees s); the new Lagrange basis is one generator and n - 1 identities,
    and the structural check of verify_srs_update says so"""
    from ezkl_amd import backend as B
    k, s = 6, S_WIDE
    t = SR.omega(k) * pow(s, -1, R) % R
    assert pow(s * t, 1 << k, R) == 1
    old = made(k, s)
    new, proof = B.update_srs(old, t)
    ident = ~new["g_lagrange"].any(axis=1)
    assert ident.sum() == (1 << k) - 1 and (new["g_lagrange"][1] == SR.G).all()
    rep = B.verify_srs_update(old, new, proof, seed=5)
    assert not rep["ok"] and rep["reason"] == "new: degenerate set: 63 identities"


# ------------------------------------------------------------------ the front doors, on files
def test_update_and_verify_on_files(hip, made, tmp_path, monkeypatch):
    import hashlib
    from ezkl_amd import execute as X
    monkeypatch.delenv("EZKL_SRS_CHECK", raising=False)
    old = made(6, S_WIDE)
    new_path = str(tmp_path / "updated.srs")
    info = X.update_srs(old["path"], new_path, secret=T_WIDE)
    raw = open(new_path, "rb").read()
    assert raw == made(6, S_WIDE * T_WIDE % R)["raw"]
    assert info == dict(k=6, t_g2=made(4, T_WIDE)["s_g2"].hex(), sha256_in=hashlib.sha256(old["raw"]).hexdigest(), sha256_out=hashlib.sha256(raw).hexdigest())
    assert X.verify_srs_update(old["path"], new_path, info["t_g2"])["ok"]
    assert X.verify_srs_update(old["path"], new_path, bytes.fromhex(info["t_g2"]))["ok"]
    with pytest.raises(X.SrsError, match="^link:") as e:
        X.verify_srs_update(new_path, old["path"], info["t_g2"])
    assert e.value.report["link"] is False
    # a drawn secret: nobody is told it, and the update still verifies
    drawn_path = str(tmp_path / "drawn.srs")
    drawn = X.update_srs(new_path, drawn_path)
    assert set(drawn) == {"k", "t_g2", "sha256_in", "sha256_out"} and drawn["sha256_in"] == info["sha256_out"] != drawn["sha256_out"]
    assert X.verify_srs_update(new_path, drawn_path, drawn["t_g2"])["ok"]
    # the input is read as the loaders read it: a bad point is refused under the default policy, nothing is written
    bad = bytearray(old["raw"]); bad[4 + 64 * 9] ^= 1
    (tmp_path / "bad.srs").write_bytes(bytes(bad))
    with pytest.raises(X.SrsError, match=r"g\[9\]"):
        X.update_srs(str(tmp_path / "bad.srs"), str(tmp_path / "never.srs"), secret=3)
    assert not (tmp_path / "never.srs").exists()


def test_a_proof_under_an_updated_srs_and_one_made_before_the_update(hip, tmp_path, monkeypatch):
    """the k = 6 test file, whose secret nobody here knows, updated and verified; setup / prove / verify of the k = 6 MLP pass under the
    new file, and a proof made under the old file verifies under the old file only"""
    from ezkl_amd import execute as X
    monkeypatch.delenv("EZKL_SRS_CHECK", raising=False)
    g = lambda name: os.path.join(FX.G, name)
    old_path, new_path = g("kzg_k6.srs"), str(tmp_path / "kzg_k6.updated.srs")
    info = X.update_srs(old_path, new_path, secret=T_WIDE)
    assert X.verify_srs_update(old_path, new_path, info["t_g2"])["ok"]
    compiled, made = g("model_k6.compiled"), {}
    for name, srs in (("old", old_path), ("new", new_path)):
        vk, pk, proof = (str(tmp_path / (name + ext)) for ext in (".vk.key", ".pk.key", ".proof.json"))
        X.setup(compiled, srs, vk, pk)
        X.prove(g("witness_k6.json"), compiled, pk, proof, srs, seed=1)
        assert X.verify(proof, compiled, vk, srs)
        made[name] = (vk, proof)
    (vk_old, proof_old), (vk_new, proof_new) = made["old"], made["new"]
    assert not X.verify(proof_old, compiled, vk_new, new_path)         # the old proof against the new key and file
    assert not X.verify(proof_old, compiled, vk_old, new_path)         # ... against its own key and the new file's s_g2
    assert not X.verify(proof_new, compiled, vk_new, old_path)
