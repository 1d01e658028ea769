"""GPU parity of the G2 set check (backend.g2_check_points: ezkl_hip_g2_check_dev, g2_check_kernel in csrc/g2.hip) with the definitions in
Python integers (tests/g2_check_ref.py: range, twist equation, [r]P == O by double-and-add).  Exact: the four words are integers."""
import numpy as np
import pytest

import g2_check_ref as G

pytestmark = pytest.mark.gpu
# one lane, the wave edges, more than one workgroup, 4097, and 65537: one point more than a one-workgroup-per-CU grid of 256 CUs has lanes,
# so that a lane strides twice and reads the record it loaded ahead (4097 does not outgrow that grid)
SIZES = [1, 63, 64, 65, 257, 4097, 65537]
CASES = ["good", "identities", "two"] + ["%s@%s" % (w, at) for w in (1, 2, 3) for at in ("first", "last", "middle")]


@pytest.fixture(scope="module")
def pool():
    """64 good records ([s]g2, each held to [r]P == O here, once) and one bad record per reason, whose twist points are held to [r]P != O"""
    good = G.good_points(64)
    assert all(G.on_curve(p) and G.in_subgroup(p) for p in good)
    bad = {w: [G.bad_record(w, s) for s in (0, 1)] for w in (1, 2, 3)}
    assert all(G.reason(r) == (w, False) for w in bad for r in bad[w])            # reason 3: on the curve and [r]P != O
    return np.stack([G.encode(p) for p in good]), bad


def _build(pool, n, case):
    """-> (the set, the rows of it that are not the pool's good records)"""
    good, bad = pool
    pts, at = good[np.arange(n) % 64].copy(), {"first": 0, "last": n - 1, "middle": n // 2}
    if case == "identities":
        placed = {0: G.encode(None), n - 1: G.encode(None)}
    elif case == "two":                                                            # the later one would win on the reason alone
        placed = {n // 3: bad[3][0], n - 1: bad[1][0]}
    elif case != "good":
        w, where = case.split("@")
        placed = {at[where]: bad[int(w)][1]}
    else:
        placed = {}
    for i, rec in placed.items():
        pts[i] = rec
    return pts, placed


@pytest.mark.parametrize("n,case", [(n, c) for n in SIZES for c in CASES if not (n == 1 and c == "two")])
def test_the_four_words_equal_the_definition(hip, pool, n, case):
    from ezkl_amd import backend as B
    pts, placed = _build(pool, n, case)
    want = G.classify(pts, known_good=set(range(n)) - set(placed))
    assert want["bad"] == (0 if case in ("good", "identities") else len(placed)) and want["identities"] == (len(placed) if case == "identities" else 0)
    got = B.g2_check_points(pts)
    print(n, case, got)
    assert got == want


def test_msm_g2_points_with_check_refuses_by_name_and_changes_nothing_on_a_good_set(hip, pool):
    from ezkl_amd import backend as B
    from conftest import rand_fr
    good, bad = pool
    pts = good[np.arange(65) % 64].copy()
    ds, dp = B.DeviceBuffer.from_numpy(rand_fr(np.random.default_rng(5), 65)), B.DeviceBuffer.from_numpy(pts)
    pts[40] = bad[3][0]
    db = B.DeviceBuffer.from_numpy(pts)
    try:
        assert B.msm_g2_points(dp, ds, check=True).tobytes() == B.msm_g2_points(dp, ds).tobytes()
        with pytest.raises(B.G2PointError, match=r"^g2\[40\]: point not in the subgroup$"):
            B.msm_g2_points(db, ds, check=True)
    finally:
        ds.free(); dp.free(); db.free()
