"""GPU parity of the MSM sort FRONT END against the oracle: the reduction-only from_mont (field.hpp: Field::redc), the signed-digit recoder
on a limb-walking bit buffer (msm.hip: msm_recode), the histogram pass, the column scan with four columns per workgroup and the persistent
partition pass that takes its raw counts from row differences.  Every result is compared with oracle.binding.msm on the same points and
scalars, and every case runs twice into the same call slot and must give the same point both times (a counter or cursor that is not
re-initialised between tiles or calls shows up there).

Values: the edges of the recoding and of the reduction -- see _edge_values.  Sizes, with the plan and the tiling each one runs at
(msm_plan.hpp: pick_plan and msm_plan; tests/cpp/test_msm_plan.cpp pins this table and the geometry at every other size without a device):
    1            W = 64 windows of 4 / 3 bits, one tile
    255          W = 29, one tile of 448 scalars, partly filled
    512, 513     W = 26: exactly one tile of 512, and one tile plus one scalar
    1024, 1025   W = 24: two full tiles of 512, and two tiles plus one scalar
    4097         W = 20: seven tiles of 640
    2^18 + 1025  W = 15: 317 tiles of 832 scalars for the 256 persistent workgroups of the partition pass on a 256-CU device, so 61 of them
                 take a second tile and 195 take one.  (The smallest size with a 257th tile is 212 993, under the same plan; this one leaves
                 a mix of one-tile and two-tile workgroups and a last tile that is partly filled.)"""
import numpy as np
import pytest
from conftest import R, SEED, fe_from_int, rand_fr
from oracle import binding as ob
from test_gpu_msm_groups import _column as _groups_column

pytestmark = pytest.mark.gpu

SIZES = (1, 255, 512, 513, 1024, 1025, 4097, (1 << 18) + 1025)
KINDS = ("uniform", "witness20", "constant", "zeros", "minus_one", "booleans")
TOP_ONES = (0x30644e71 << 224) | ((1 << 224) - 1)        # every limb 0xffffffff below the top one, the top one the modulus's less one: < r


def _column(kind, rng, n):
    if kind == "booleans":                                   # every pair in bucket 0's own partition
        return np.stack([np.zeros(4, np.uint64), fe_from_int(1)])[rng.integers(0, 2, n)]
    return _groups_column(kind, rng, n)


def _edge_values():
    """canonical scalars at the edges of the recoding: 0, 1, 2, r - 1, r - 2; the two sides of the negation fold; 2^k - 1, 2^k, 2^k + 1 for
    every k (every window edge of every plan, carries that run through all windows, digits equal to half a window); all-ones limbs"""
    v = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2]
    for k in range(1, 254):
        v += [(1 << k) - 1, 1 << k, (1 << k) + 1]
    v.append(TOP_ONES)
    return list(dict.fromkeys(v))


_EDGES = {}


def _edges():
    """(column, points, bases, device column, oracle result per value) on ONE point, plus 64 uniform values and the scalar whose MONTGOMERY
    form has the all-ones limbs (the input edge of the reduction); made once"""
    from ezkl_amd import backend as B
    if not _EDGES:
        rng = np.random.default_rng(77)
        col = np.stack([fe_from_int(x) for x in _edge_values()] + [np.frombuffer(TOP_ONES.to_bytes(32, "little"), np.uint64)])
        col = np.concatenate([col, rand_fr(rng, 64)])
        pts = ob.gen_bases(SEED + 21, 1)
        want = np.stack([ob.msm(col[i:i + 1], pts) for i in range(len(col))])
        _EDGES["v"] = (col, pts, B.Bases(pts), B.DeviceBuffer.from_numpy(col), want)
    return _EDGES["v"]


_SETS = {}
_WANT = {}


def _set(n):
    """(points, bases) for n points: made once, shared, never modified"""
    from ezkl_amd import backend as B
    if n not in _SETS:
        pts = ob.gen_bases(SEED + 22, n)
        _SETS[n] = (pts, B.Bases(pts))
    return _SETS[n]


def _case(n, kind):
    """(device column, oracle result) of one kind at one size: made once"""
    from ezkl_amd import backend as B
    if (n, kind) not in _WANT:
        col = _column(kind, np.random.default_rng(2000 + n + KINDS.index(kind)), n)
        _WANT[(n, kind)] = (B.DeviceBuffer.from_numpy(col), ob.msm(col, _set(n)[0]))
    return _WANT[(n, kind)]


def test_value_edges_one_scalar_at_a_time(hip):
    """n = 1 (64 windows of 4 / 3 bits): one call per value"""
    from ezkl_amd import backend as B
    col, _, bases, dev, want = _edges()
    bad = []
    for i in range(len(col)):
        for run in range(2):
            if not (B.msm_g1_dev(bases, dev.ptr + 32 * i, 1) == want[i]).all():
                bad.append((i, run))
    assert not bad, bad[:20]


def test_value_edges_in_one_column(hip):
    """the same values together in one 1024-scalar column (two tiles, W = 24), filled up with uniform values"""
    from ezkl_amd import backend as B
    n = 1024
    col = _edges()[0]
    assert len(col) <= n
    col = np.concatenate([col, rand_fr(np.random.default_rng(78), n - len(col))])
    pts, bases = _set(n)
    want = ob.msm(col, pts)
    dev = B.DeviceBuffer.from_numpy(col)
    for run in range(2):
        assert (B.msm_g1_dev(bases, dev.ptr, n) == want).all(), run


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_column_kinds(hip, n, kind):
    from ezkl_amd import backend as B
    dev, want = _case(n, kind)
    bases = _set(n)[1]
    for run in range(2):
        assert (B.msm_g1_dev(bases, dev.ptr, n) == want).all(), (n, kind, run)


@pytest.mark.parametrize("n", [1025, 4097])
@pytest.mark.parametrize("batch", [2, 5, 16])
def test_fused_groups(hip, monkeypatch, n, batch):
    """columns of different kinds in one fused group (gridDim.z = batch): the row differences and the persistent loop work on per-column slabs"""
    from ezkl_amd import backend as B
    monkeypatch.setenv("EZKL_MSM_GROUP", "16")
    kinds = [KINDS[(j + batch) % len(KINDS)] for j in range(batch)]
    cases = [_case(n, k) for k in kinds]
    bases = _set(n)[1]
    for run in range(2):
        got = B.msm_g1_batch_dev(bases, [d.ptr for d, _ in cases], n)
        for j, (_, want) in enumerate(cases):
            assert (got[j] == want).all(), (n, batch, j, kinds[j], run)
