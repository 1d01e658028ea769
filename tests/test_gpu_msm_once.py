"""GPU parity of the MSM without window tables (Bases.msm_once, backend.msm_points: ezkl_hip_msm_g1_once_dev / _points_dev) with the fixed-base
MSM on the same inputs, byte for byte, and for a subset with the oracle's MSM: sizes past one wave, one partition tile (1024 scalars) and
one accumulate round; scalars at the edges of the recoding (the r - s fold, carries through every window, empty windows, one bucket for
everything); degenerate points; base offsets; the entry points' contract; and that backend.check_srs no longer builds a table."""
import ctypes as C

import numpy as np
import pytest

from conftest import Q, R, SEED, fe_from_int, rand_fr
from oracle import binding as ob

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 257, 1000, 4097, (1 << 14) + 3]
EZKL_ERR_INVALID = -3            # include/ezkl_hip.h


def _plan_once(n):
    """(W, base, rem) of csrc/msm_plan.hpp's pick_plan_once, restated: it only aims the carry patterns below at the window edges"""
    best = None
    for W in range(12, 128):
        base, rem = divmod(254, W)
        cmax = base + (1 if rem else 0)
        if cmax > 23:
            continue
        cost = W * (n + 4 * (1 << (cmax - 1))) + ((W + 15) // 16) * (1 << 22)
        if best is None or cost < best[0]:
            best = (cost, W, base, rem)
    return best[1:]


def _col(values):
    return np.stack([fe_from_int(int(v) % R) for v in values])


@pytest.fixture(scope="module")
def sets(hip):
    """n -> (a resident set of n generated points, its records): made once, freed with the module; the fixed-base side builds its tables
    at the first comparison"""
    from ezkl_amd import backend as B
    cache = {}
    def get(n):
        if n not in cache:
            b = B.Bases.generate(SEED + 7, n)
            pts = b.download()
            pts.setflags(write=False)
            cache[n] = (b, pts)
        return cache[n]
    yield get
    for b, _ in cache.values():
        b.free()


def _both(b, scalars, first=0, n=None):
    """(table-free, fixed-base) on the same resident scalars"""
    from ezkl_amd import backend as B
    d = B.DeviceBuffer.from_numpy(np.ascontiguousarray(scalars))
    try:
        return b.msm_once(d.ptr, first, n), b.msm(d.ptr, first, n)
    finally:
        d.free()


def _same(b, scalars, pts=None, first=0, n=None):
    once, fixed = _both(b, scalars, first, n)
    assert once.tobytes() == fixed.tobytes()
    if pts is not None:
        m = len(scalars) if n is None else n
        assert once.tobytes() == ob.msm(np.ascontiguousarray(scalars[:m]), np.ascontiguousarray(pts[first:first + m])).tobytes()
    return once


@pytest.mark.parametrize("n", SIZES)
def test_uniform_scalars_at_every_size(hip, n):
    from ezkl_amd import backend as B
    b = B.Bases.generate(SEED + 7, n)             # a set of this test's own: nothing else has touched the handle
    pts = b.download()
    s = rand_fr(np.random.default_rng(n), n)
    d = B.DeviceBuffer.from_numpy(s)
    try:
        assert not b.has_table()
        once = b.msm_once(d.ptr)
        assert not b.has_table()                  # and the table-free call left it without one
        assert B.last_kernel_ms("msm_once") > 0
        assert once.tobytes() == b.msm(d.ptr).tobytes()
        assert b.has_table()
        assert once.tobytes() == b.msm_once(d.ptr).tobytes()        # a handle that has a table: the call ignores it
    finally:
        d.free(); b.free()
    assert once.tobytes() == ob.msm(s, np.ascontiguousarray(pts)).tobytes()


def _edge_scalars(n):
    W, base, rem = _plan_once(n)
    width = lambda w: base + (1 if w < rem else 0)
    offset = lambda w: w * base + min(w, rem)
    all_ones = (1 << 252) - 1                      # every window 2^c - 1 below the fold: each digit is -1 or 0 with a carry, up into the top window
    half_plus = 0
    for w in range(W):
        for bit in (offset(w), offset(w) + width(w) - 1):
            if bit < 252:
                half_plus |= 1 << bit              # every window 2^(c-1) + 1: just past the half, a negative digit and a carry
    rng = np.random.default_rng(20)
    small = rng.integers(-(1 << 20) + 1, 1 << 20, size=n)
    small[rng.random(n) < 0.2] = 0
    return dict(
        zero=np.zeros((n, 4), np.uint64),
        one=np.tile(fe_from_int(1), (n, 1)),
        minus_one=np.tile(fe_from_int(R - 1), (n, 1)),
        half_r=_col([(R - 1) // 2 if i % 2 else (R + 1) // 2 for i in range(n)]),
        all_ones=_col([all_ones if i % 2 else R - all_ones for i in range(n)]),
        half_plus=_col([half_plus if i % 3 else R - half_plus for i in range(n)]),
        witness_like=_col(small),
    )


@pytest.mark.parametrize("n", [65, 4097])
@pytest.mark.parametrize("kind", ["zero", "one", "minus_one", "half_r", "all_ones", "half_plus", "witness_like"])
def test_scalars_at_the_edges_of_the_recoding(hip, sets, n, kind):
    """zero: every window empty; one: n pairs in ONE bucket of window 0 (the heavy fix-ups) and every other member of the fused group empty;
    minus_one: the same after the fold; half_r: both sides of the fold; all_ones / half_plus: carries through every window"""
    b, pts = sets(n)
    once = _same(b, _edge_scalars(n)[kind], pts)
    if kind == "zero":
        assert not once.any()


def _neg(p):
    out = p.copy()
    out[4:] = np.frombuffer(((Q - int.from_bytes(p[4:].tobytes(), "little")) % Q).to_bytes(32, "little"), np.uint64)
    return out


def test_degenerate_points(hip, sets):
    from ezkl_amd import backend as B
    _, base = sets(4097)
    n = 4096
    rng = np.random.default_rng(31)
    # every record the same point: the additions inside a bucket and in the trees are doublings
    same = B.Bases(np.tile(base[3], (n, 1)))
    # P, -P, P, -P, ... under equal scalars: the sum is the identity
    pm = np.tile(base[5], (n, 1))
    pm[1::2] = _neg(base[5])
    cancel = B.Bases(pm)
    # identities among the points
    holes = base[:n].copy()
    holes[[0, 1, 63, 64, 1023, 1024, n - 1]] = 0
    holes[rng.random(n) < 0.1] = 0
    holed = B.Bases(holes)
    try:
        for s in (rand_fr(rng, n), np.tile(fe_from_int(7), (n, 1)), np.tile(fe_from_int(R - 7), (n, 1))):
            _same(same, s, np.tile(base[3], (n, 1)))
            assert not _same(cancel, np.repeat(s[::2], 2, axis=0)).any()
            _same(holed, s, holes)
    finally:
        same.free(); cancel.free(); holed.free()


def test_golden_srs(hip, golden_srs, golden_pk):
    from ezkl_amd import backend as B
    g, gl = B.Bases(golden_srs["g"]), B.Bases(golden_srs["g_lagrange"])
    try:
        for v, p in zip(golden_pk["fixed_values"], golden_pk["fixed_polys"]):
            a = _same(gl, v, golden_srs["g_lagrange"])
            assert a.tobytes() == _same(g, p, golden_srs["g"]).tobytes()         # commit_lagrange(v) == commit(iNTT v)
        ones = np.tile(fe_from_int(1), (64, 1))
        assert _same(gl, ones).tobytes() == golden_srs["g"][0].tobytes()          # the Lagrange basis sums to g[0]
    finally:
        g.free(); gl.free()


@pytest.mark.parametrize("n", [65, 1000])
def test_base_offsets(hip, sets, n):
    """offsets 0, 1 (odd: check_srs uses it) and n / 2 into a set of 2 n points"""
    b, pts = sets(2 * n)
    s = rand_fr(np.random.default_rng(n + 1), n)
    seen = set()
    for first in (0, 1, n // 2, n):
        seen.add(_same(b, s, pts, first, n).tobytes())
    assert len(seen) == 4


def test_points_that_are_no_base_set(hip, sets):
    from ezkl_amd import backend as B
    for n in (65, 4097):
        b, pts = sets(n)
        s = rand_fr(np.random.default_rng(n + 2), n)
        dp, ds = B.DeviceBuffer.from_numpy(np.ascontiguousarray(pts)), B.DeviceBuffer.from_numpy(s)
        try:
            got = B.msm_points(dp.ptr, ds.ptr, n)
            assert got.tobytes() == b.msm_once(ds.ptr).tobytes() == ob.msm(s, np.ascontiguousarray(pts)).tobytes()
            assert B.msm_points(dp.ptr + 64, ds.ptr, n - 1).tobytes() == b.msm_once(ds.ptr, 1, n - 1).tobytes()
            assert dp.to_numpy(shape=(n, 8)).tobytes() == pts.tobytes()        # the caller's points are read, never written
        finally:
            dp.free(); ds.free()


def test_errors(hip, sets):
    from ezkl_amd import backend as B, lib as L
    b, _ = sets(65)
    d = B.DeviceBuffer.from_numpy(rand_fr(np.random.default_rng(3), 65))
    out = np.zeros(8, np.uint64)
    def once(first, n, scalars=d.ptr, h=b.h):
        return L.load().ezkl_hip_msm_g1_once_dev(h, C.c_size_t(first), C.c_void_p(scalars), C.c_size_t(n), out.ctypes.data_as(C.c_void_p), None)
    try:
        assert once(0, 65) == 0
        assert once(0, 0) == EZKL_ERR_INVALID
        assert once(0, 66) == once(1, 65) == once(65, 1) == once(66, 0) == once(2**63, 2**63) == EZKL_ERR_INVALID
        assert once(0, 65, scalars=None) == once(0, 65, h=None) == EZKL_ERR_INVALID
        pts = L.load().ezkl_hip_msm_g1_points_dev
        assert pts(C.c_void_p(d.ptr), C.c_void_p(d.ptr), C.c_size_t(0), out.ctypes.data_as(C.c_void_p), None) == EZKL_ERR_INVALID
        assert pts(None, C.c_void_p(d.ptr), C.c_size_t(1), out.ctypes.data_as(C.c_void_p), None) == EZKL_ERR_INVALID
        with pytest.raises(L.EzklHipError) as e:
            b.msm_once(d.ptr, 0, 0)
        assert e.value.code == EZKL_ERR_INVALID
        with pytest.raises(ValueError):
            b.msm_once(d.ptr, 1, 65)
        assert once(64, 1) == 0                                                # the last record alone
    finally:
        d.free()


def test_table_state_and_scratch_reuse(hip):
    from ezkl_amd import backend as B
    big, small = (1 << 14) + 3, 65
    b = B.Bases(ob.gen_bases(SEED + 9, big))                                   # uploaded, not generated on the device
    d = B.DeviceBuffer.from_numpy(rand_fr(np.random.default_rng(9), big))
    try:
        first = b.msm_once(d.ptr)
        assert not b.has_table()
        free0 = B.mem_info()[0]
        a = b.msm_once(d.ptr, 0, small)                                        # a smaller one, the large one again: no allocation
        assert b.msm_once(d.ptr).tobytes() == first.tobytes()
        assert B.mem_info()[0] == free0 and not b.has_table()
        b.prepare()
        assert b.has_table()
        assert b.msm(d.ptr).tobytes() == first.tobytes() == b.msm_once(d.ptr).tobytes()
        assert b.msm(d.ptr, 0, small).tobytes() == a.tobytes()
    finally:
        d.free(); b.free()


def test_check_srs_builds_no_table(hip, tmp_path, monkeypatch):
    """backend.check_srs on a k = 8 file: three MSMs, and neither set ever has a window table; the same call with the switch
    (MSM_ONCE_MIN_POINTS) set past every size builds them and reports the same"""
    from ezkl_amd import backend as B, codecs, execute as X
    path = str(tmp_path / "kzg8.srs")
    X.gen_srs(path, 8, secret=0x1234567)
    srs = codecs.read_srs(open(path, "rb").read())
    seen = []
    free = B._Bases.free
    def watched(self):
        if self.h:
            seen.append(self.has_table())
        free(self)
    monkeypatch.setattr(B._Bases, "free", watched)
    rep = B.check_srs(srs, seed=3)
    assert rep["ok"] and rep["powers"] is rep["lagrange"] is True, rep
    assert seen == [False, False]
    bad = dict(srs, g_lagrange=srs["g_lagrange"].copy())
    bad["g_lagrange"][200] = ob.g1_add(bad["g_lagrange"][200], bad["g_lagrange"][200])
    rep_bad = B.check_srs(bad, seed=3)
    assert not rep_bad["ok"] and rep_bad["powers"] is True and rep_bad["lagrange"] is False
    del seen[:]
    monkeypatch.setattr(B, "MSM_ONCE_MIN_POINTS", 1 << 62)
    assert B.check_srs(srs, seed=3) == rep and B.check_srs(bad, seed=3) == rep_bad
    assert seen == [True, True, True, True]
