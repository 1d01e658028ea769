"""GPU parity of the three device paths that build the structured reference string: g1_mul_fixed_kernel (Bases.from_scalars, gen_srs),
the inverse NTT over G1 (ecntt_* in msm.hip: Bases.downsize, every load_params_prover whose SRS file is larger than the circuit) and the
G2 fold (g2.hip).  Every comparison is exact byte equality against the oracle (oracle.binding: double-and-add, its CPU MSM and FFT) or
against tests/srs_ref.py (Python integers + the oracle's double-and-add); the device's MSM and NTT are a reference nowhere in this file.

Which comparisons are over the whole output and which are sampled is said in each test's docstring; a sampled one always comes with
srs_ref.functional_check over the whole set (commit_lagrange(v) == commit(iNTT v) on the host), which a single wrong point fails."""
import numpy as np
import pytest
from conftest import R, Q, SEED, fe_from_int, fe_to_int, rand_fr
from oracle import binding as ob
import srs_ref as SR

pytestmark = pytest.mark.gpu

S = 0x1234567890abcdef1234567890abcdef % R                   # an ordinary secret
ALL_ONES = lambda bits, shift: ((1 << bits) - 1) << shift
# scalar edges of the double-and-add over the canonical bits 253 .. 0 (r is a 254-bit number: r - 1 is the largest canonical value, and
# it has bit 253 set); the first five have bit 253 set
EDGES = [R - 1, 1 << 253, (1 << 253) + 1, R - 2, (1 << 253) + (1 << 252) - 1,
         (1 << 253) - 1, 0, 1, 2, 3, (R - 1) // 2, (R + 1) // 2, (1 << 32) - 1, 1 << 32, 1 << 224,
         ALL_ONES(16, 24), ALL_ONES(64, 32), ALL_ONES(100, 60), ALL_ONES(40, 108), ALL_ONES(33, 191), ALL_ONES(3, 223)]
assert all(0 <= e < R for e in EDGES) and sum(e >> 253 for e in EDGES) == 5


def _brev(i, k):
    return int(format(i, "0%db" % k)[::-1], 2) if k else 0


def _bad_rows(got, want):
    return np.flatnonzero((np.asarray(got) != np.asarray(want)).any(axis=1)).tolist()


def _scalar_column(n, seed):
    """uniform values of Fr (a third of them have bit 253 set) with EDGES planted at rows 0, 255, 256, n - 1 and spread in between -> (canonical ints, edge rows)"""
    col = [fe_to_int(v) for v in rand_fr(np.random.default_rng(seed), n)]
    if n == 1:
        return [R - 1], [0]
    rows = [r for r in (0, 255, 256, n - 1) if r < n]
    rows += [int(r) for r in np.linspace(1, n - 2, len(EDGES)).round() if int(r) not in rows]
    for j, r in enumerate(dict.fromkeys(rows)):
        col[r] = EDGES[j % len(EDGES)]
    assert n < len(EDGES) or set(EDGES) <= set(col)
    return col, rows


@pytest.fixture(scope="module")
def other_point():
    return ob.gen_bases(SEED + 11, 3)[2]


@pytest.mark.parametrize("base", ["generator", "other", "identity"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
def test_from_scalars_matches_double_and_add(hip, other_point, n, base):
    """g1_mul_fixed_kernel (Bases.from_scalars): EVERY row against oracle.binding.g1_mul, at lengths around one workgroup of 256 and past
    four, scalars at the edges of the bit loop (0, 1, r - 1, bit 253 set, runs of ones across the limbs) on the rows at the workgroup
    edges, for the generator, an arbitrary point and the identity as base (every output is then the identity)."""
    from ezkl_amd import backend as B
    col, _ = _scalar_column(n, n)
    P = {"generator": SR.G, "other": other_point, "identity": np.zeros(8, np.uint64)}[base]
    dev = B.DeviceBuffer.from_numpy(SR.fes(col))
    b = B.Bases.from_scalars(P, dev.ptr, n)
    got = b.download()
    b.free(); dev.free()
    assert got.shape == (n, 8)
    if base == "identity":
        assert not got.any()
        return
    bad = _bad_rows(got, SR.mul_many(P, col))
    assert not bad, "rows %s differ; of these, bit 253 of the scalar is set at %s" % (bad, [r for r in bad if col[r] >> 253])
    assert not got[[r for r in range(n) if col[r] == 0]].any()


def _downsize(B, g_host, k2):
    bg = B.Bases(g_host)
    dg, dl = bg.downsize(k2)
    out = dg.download(), dl.download()
    for b in (bg, dg, dl): b.free()
    return out


@pytest.mark.parametrize("k2", [9, 10, 11])
def test_downsize_of_a_structured_set_whole_output(hip, k2):
    """ecntt_* at one workgroup of butterflies (k' = 9: 256 threads) and past it (k' = 10, 11: t >= 256 in the blk / j / lo / hi
    arithmetic): oracle-made g = [s^i] G uploaded, ALL 2^k' points of both returned sets against srs_ref.structured_set."""
    from ezkl_amd import backend as B
    g, gl = SR.structured_set(S, k2)
    got_g, got_gl = _downsize(B, g, k2)
    assert got_g.tobytes() == g.tobytes()
    assert not _bad_rows(got_gl, gl)


def test_downsize_at_k13_many_workgroups_and_a_chunked_twiddle_scan(hip):
    """k' = 13: 16 workgroups per stage and a twiddle column of 4096 > one scan chunk.  g comes from from_scalars (pinned above, and again
    here on the sampled rows).  SAMPLED: rows 0, 255, 256, 257, 4095, 4096, n' - 1 and 256 seeded random rows of g_lagrange against
    [L_i(s)] G by double-and-add; WHOLE SET: g' == g, and the functional check over all 8192 points."""
    from ezkl_amd import backend as B
    k2, n = 13, 1 << 13
    dev = B.DeviceBuffer.from_numpy(SR.fes(SR.power_scalars(S, n)))
    bg = B.Bases.from_scalars(SR.G, dev.ptr, n)
    dg, dl = bg.downsize(k2)
    g, got_g, got_gl = bg.download(), dg.download(), dl.download()
    for b in (bg, dg, dl): b.free()
    dev.free()
    rows = sorted({0, 255, 256, 257, 4095, 4096, n - 1} | {int(r) for r in np.random.default_rng(13).choice(n, 256, replace=False)})
    assert len(rows) >= 256
    c, p = SR.lagrange_scalars(S, k2), SR.power_scalars(S, n)
    assert not _bad_rows(g[rows], SR.mul_many(SR.G, [p[r] for r in rows]))
    assert got_g.tobytes() == g.tobytes()
    assert not _bad_rows(got_gl[rows], SR.mul_many(SR.G, [c[r] for r in rows]))
    assert SR.functional_check(g, got_gl, k2, seed=13)


@pytest.mark.parametrize("name", ["zero", "one", "w5"])
def test_downsize_with_a_degenerate_secret_whole_output(hip, name):
    """the branches a well-formed SRS never takes, k' = 10, ALL rows: s = 0 (g = G then identities: identities through every
    g1x_scalar_mul and g1x_add, the result [1/n] G in every row), s = 1 (g = G everywhere: every stage-1 butterfly adds equal points --
    g1x_add falling into g1x_double -- and subtracts them -- the identity), s = w^5 (one G and n' - 1 identities come out)."""
    from ezkl_amd import backend as B
    k2, n = 10, 1 << 10
    s = {"zero": 0, "one": 1, "w5": pow(SR.omega(k2), 5, R)}[name]
    g, gl = SR.structured_set(s, k2)
    got_g, got_gl = _downsize(B, g, k2)
    assert got_g.tobytes() == g.tobytes()
    assert not _bad_rows(got_gl, gl)
    ident = ~got_gl.any(axis=1)
    if name == "zero":
        assert not g[1:].any() and not ident.any() and (got_gl == ob.g1_mul(SR.G, SR.fe(pow(n, -1, R)))).all()
    else:
        row = 0 if name == "one" else 5
        assert ident.sum() == n - 1 and (got_gl[row] == SR.G).all()


def test_downsize_from_a_larger_source_set_whole_output(hip):
    """12 -> 10: truncation together with the transform (what load_params_prover does with a shared SRS file), ALL rows of both sets"""
    from ezkl_amd import backend as B
    g12 = SR.powers_set(S, 12)
    g, gl = SR.structured_set(S, 10)
    assert g12[:1024].tobytes() == g.tobytes()
    got_g, got_gl = _downsize(B, g12, 10)
    assert got_g.tobytes() == g.tobytes()
    assert not _bad_rows(got_gl, gl)


def _planted_set(k2):
    """gen_bases points with the G1 NTT's rare branches planted.  g[x] and g[x + n/2] are the two inputs of one stage-1 butterfly (they
    sit next to each other after the bit-reversed load; the twiddle is 1): equal points make it double and cancel, opposite points
    cancel and double, identities pass through.  -> (g, the x of every planted butterfly)"""
    n, h = 1 << k2, 1 << (k2 - 1)
    g = ob.gen_bases(SEED + 7, n).copy()
    dup = [0, 3, h // 2 - 1, h // 2 + 44, h - 1]
    opp = [1, h // 2, h // 2 + 1, h - 112]
    for x in dup:
        g[x + h] = g[x]
    for y in opp:
        g[y + h] = SR.neg(g[y])
    g[7] = 0                                                  # an identity in the lower half, one in the upper, both halves of one butterfly
    g[h + h // 4] = 0
    g[20] = 0; g[20 + h] = 0
    run = list(range(h // 8, h // 8 + 64))                    # a run of 64 identities
    g[run] = 0
    return g, dup + opp + [7, h // 4, 20] + run


def _row_reference(g, k2, i):
    e = np.zeros((1 << k2, 4), np.uint64)
    e[i] = fe_from_int(1)
    return ob.msm(ob.lagrange_to_coeff(e, k2), g)


def test_downsize_of_an_unstructured_set_with_planted_branches(hip):
    """k' = 10 on gen_bases points with equal / opposite stage-1 partners, isolated identities and a run of 64 (the curve.hpp XYZZ forms
    of g1x_add's doubling and cancelling branches, and identities through g1x_scalar_mul).  SAMPLED against the oracle's MSM of the
    Lagrange polynomial's coefficients (one MSM per row): the rows at every workgroup edge, both rows of every stage-1 butterfly that
    holds a planted point and the planted inputs' own rows, 32 seeded random rows; WHOLE SET: g' == g and the functional check."""
    from ezkl_amd import backend as B
    k2, n, h = 10, 1 << 10, 1 << 9
    g, planted = _planted_set(k2)
    got_g, got_gl = _downsize(B, g, k2)
    assert got_g.tobytes() == g.tobytes()
    rows = {0, n - 1} | {e + d for e in range(256, n, 256) for d in (-1, 0, 1)}
    for x in planted:
        rows |= {_brev(x, k2), _brev(x, k2) + 1}
    for x in planted[:12]:
        rows |= {x, x + h}
    rows |= {int(r) for r in np.random.default_rng(10).choice(n, 32, replace=False)}
    rows = sorted(rows)
    assert len(rows) >= 2 * len(planted) and max(rows) < n
    want = np.stack([_row_reference(g, k2, i) for i in rows])
    bad = [rows[j] for j in _bad_rows(got_gl[rows], want)]
    assert not bad, "rows %s of %d compared differ" % (bad, len(rows))
    assert SR.functional_check(g, got_gl, k2, seed=10)


def test_downsize_of_an_unstructured_set_at_k8_whole_output(hip):
    """the same construction at k' = 8, ALL rows against the oracle's g1_to_lagrange, plus the functional check"""
    from ezkl_amd import backend as B
    g, _ = _planted_set(8)
    got_g, got_gl = _downsize(B, g, 8)
    assert got_g.tobytes() == g.tobytes()
    assert not _bad_rows(got_gl, ob.g1_to_lagrange(g, 8))
    assert SR.functional_check(g, got_gl, 8, seed=8)


@pytest.mark.parametrize("name", ["ordinary", "zero"])
def test_gen_srs_whole_output(hip, name):
    """backend.gen_srs at k = 10 (four workgroups of g1_mul_fixed_kernel behind the device's power scan, batch inversion and vector
    products): ALL rows of g and g_lagrange against srs_ref.structured_set.  s = 0 is legal (0^n = 0: not a point of the domain)."""
    from ezkl_amd import backend as B
    s = {"ordinary": S, "zero": 0}[name]
    g, gl = SR.structured_set(s, 10)
    bg, bgl = B.gen_srs(10, s)
    got_g, got_gl = bg.download(), bgl.download()
    bg.free(); bgl.free()
    assert not _bad_rows(got_g, g)
    assert not _bad_rows(got_gl, gl)


def test_gen_srs_refuses_a_secret_inside_the_domain(hip, tmp_path):
    """s^n = 1 (s = 1, s = w^j): the closed form is 0 / 0 at row j and every point used to come out as the identity, unreported.  Now a
    ValueError that names the reason, from backend.gen_srs and from execute.gen_srs (no file is written); s = 0 and s = w^j of a LARGER
    domain (not a point of this one) still work."""
    from ezkl_amd import backend as B, execute as X
    k = 6
    for s in (1, R + 1, SR.omega(k), pow(SR.omega(k), 37, R), R - 1):
        with pytest.raises(ValueError, match="domain"):
            B.gen_srs(k, s)
        with pytest.raises(ValueError, match="domain"):
            X.gen_srs(str(tmp_path / "bad.srs"), k, secret=s)
    assert not (tmp_path / "bad.srs").exists()
    for s in (0, SR.omega(k + 1)):
        g, gl = SR.structured_set(s, k)
        bg, bgl = B.gen_srs(k, s)
        assert bg.download().tobytes() == g.tobytes() and bgl.download().tobytes() == gl.tobytes()
        bg.free(); bgl.free()
    assert X.gen_srs(str(tmp_path / "zero.srs"), k, secret=0) == 4 + 2 * 64 * 64 + 256
    buf = (tmp_path / "zero.srs").read_bytes()
    g, gl = SR.structured_set(0, k)
    assert buf[4:4 + 64 * 64] == g.tobytes() and buf[4 + 64 * 64:4 + 2 * 64 * 64] == gl.tobytes()
    assert not any(buf[-128:])                                                      # s_g2 = [0] g2


G2 = ((0x1800deef121f1e76426a00665e5c4479674322d4f75edadd46debd5cd992f6ed, 0x198e9393920d483a7260bfb731fb5d25f1aa493335a9e71297e485b7aef312c2),
      (0x12c85ea5db8c6deb4aab71808dcb408fe3d1e7690c43d37b4ce6cc0166fa7daa, 0x090689d0585ff075ec9e99ad690c3395bc4b313370b38ef355acdadcd122975b))


def _g2_enc(pt):
    if pt is None:
        return np.zeros(16, np.uint64)
    return np.concatenate([fe_from_int(c, Q) for c in (pt[0][0], pt[0][1], pt[1][0], pt[1][1])])


def _g2_dec(a):
    v = [fe_to_int(a[4 * i:4 * i + 4], Q) for i in range(4)]
    return None if not any(v) else ((v[0], v[1]), (v[2], v[3]))


@pytest.fixture(scope="module")
def g2_multiples():
    """eight multiples of the G2 generator (the last one is the identity) -> (their discrete logs, the encoded points)"""
    from oracle import pairing as E
    ks = [int(x) for x in np.random.default_rng(2).integers(1, 1 << 40, 7)] + [0]
    return ks, np.stack([_g2_enc(E.g2_mul(G2, k) if k else None) for k in ks])


@pytest.mark.parametrize("n", [63, 64, 65, 1023, 1024, 1025])
def test_g2_msm_at_the_edges_of_its_workgroups_and_of_its_thread_count(hip, g2_multiples, n):
    """g2_msm at the edges of its 64-lane workgroups and of T = min(n, 1024) threads (thread t sums rows t, t + T, ...; one workgroup
    then folds partial[i], partial[i + 64], ...): full-width scalars on multiples of the generator picked at random, the identity among
    them, so that the expected point is one oracle scalar multiplication.  At n = 1025 row 1024 is the only non-zero scalar of thread
    0's stride; from n = 64 on, every row that lane 3 of the fold reads (3, 67, ...) is the identity."""
    from ezkl_amd import backend as B
    from oracle import pairing as E
    ks, enc = g2_multiples
    rng = np.random.default_rng(n)
    idx = rng.integers(0, 8, n)
    sc = [fe_to_int(v) for v in rand_fr(rng, n)]
    sc[n // 2], sc[n - 2] = R - 1, (1 << 253) - 1
    if n >= 64:
        for i in range(3, min(n, 1024), 64):
            if i % 128 == 3: sc[i] = 0                        # a zero scalar on a point
            else: idx[i] = 7                                  # a scalar on the identity
    if n == 1025:
        sc[0] = 0
        idx[1024], sc[1024] = 2, R - 2
    want = E.g2_mul(G2, sum(s * ks[i] for s, i in zip(sc, idx)) % R)
    got = B.msm_g2(enc[idx], SR.fes(sc))
    assert want is not None and _g2_dec(got) == want
    if n == 1025:                                             # and that row alone
        z = [0] * n; z[1024] = sc[1024]
        assert _g2_dec(B.msm_g2(enc[idx], SR.fes(z))) == E.g2_mul(G2, sc[1024] * ks[2] % R)
