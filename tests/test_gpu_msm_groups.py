"""GPU parity of FUSED MSM groups (one sequence of launches with gridDim.z = the group's columns) against the oracle: the group's scalar
columns reach the kernels by value in the kernel arguments (msm.hip: MsmCols) and every scratch pointer is shifted per column by
blockIdx.z * the slab stride -- a wrong slab offset, a swapped column pointer or a result written to the wrong place changes a point here.
Every column of a batch holds a different distribution, and the shapes are the smallest at which that code can go wrong."""
import numpy as np
import pytest
from conftest import R, SEED, fe_from_int, rand_fr
from oracle import binding as ob

pytestmark = pytest.mark.gpu

NCOLS = 17                       # 16 fill the argument struct; the 17th opens a second group
KINDS = ("uniform", "witness20", "constant", "zeros", "minus_one")


def _column(kind, rng, n):
    if kind == "uniform":
        return rand_fr(rng, n)
    if kind == "witness20":                                  # 20-bit witness-like values, a third of them zero
        v = rng.integers(1, 1 << 20, n, dtype=np.uint64)
        v[rng.random(n) < 1 / 3] = 0
        table = {}
        return np.stack([table.setdefault(int(x), fe_from_int(int(x))) for x in v])
    if kind == "constant":                                   # one value everywhere: one heavy bucket per window
        return np.tile(rand_fr(rng, 1), (n, 1))
    if kind == "zeros":
        return np.zeros((n, 4), np.uint64)
    return np.tile(fe_from_int(R - 1), (n, 1))               # r - 1 everywhere


_SETS = {}


def _set(n):
    """(points, bases, host columns, device columns, oracle results) for n points: made once, shared by every test, never modified"""
    from ezkl_amd import backend as B
    if n not in _SETS:
        rng = np.random.default_rng(1000 + n)
        pts = ob.gen_bases(SEED + 11, n)
        cols = [_column(KINDS[j % len(KINDS)], rng, n) for j in range(NCOLS)]
        want = np.stack([ob.msm(c, pts) for c in cols])
        _SETS[n] = (pts, B.Bases(pts), cols, [B.DeviceBuffer.from_numpy(c) for c in cols], want)
    return _SETS[n]


@pytest.fixture
def group16(monkeypatch):
    """fused groups of up to MSM_MAX_GROUP = 16 columns (the default is 4 / 6: EZKL_MSM_GROUP is read at every call)"""
    monkeypatch.setenv("EZKL_MSM_GROUP", "16")


@pytest.mark.parametrize("n", [1, 65, 1000, 4097])
@pytest.mark.parametrize("batch", [1, 2, 5, 16, 17])
def test_fused_groups_match_the_oracle(hip, group16, n, batch):
    """batch 1: the count == 1 path; 2, 5: partly filled argument struct; 16: full; 17: a full group and a single MSM"""
    from ezkl_amd import backend as B
    _, bases, _, devs, want = _set(n)
    got = B.msm_g1_batch_dev(bases, [d.ptr for d in devs[:batch]], n)
    assert got.shape == (batch, 8)
    for j in range(batch):
        assert (got[j] == want[j]).all(), (n, batch, j, KINDS[j % len(KINDS)])


@pytest.mark.parametrize("n", [65, 1000])
def test_default_grouping_matches_the_oracle(hip, n):
    """the same seventeen columns in the default groups of four (4 + 4 + 4 + 4 + 1 over the slot streams)"""
    from ezkl_amd import backend as B
    _, bases, _, devs, want = _set(n)
    assert (B.msm_g1_batch_dev(bases, [d.ptr for d in devs], n) == want).all()


@pytest.mark.parametrize("batch", [5, 16, 17])
def test_permuted_columns_give_permuted_results(hip, group16, batch):
    from ezkl_amd import backend as B
    n = 1000
    _, bases, _, devs, want = _set(n)
    rng = np.random.default_rng(batch)
    for _ in range(3):
        perm = rng.permutation(batch)
        got = B.msm_g1_batch_dev(bases, [devs[j].ptr for j in perm], n)
        assert (got == want[perm]).all(), perm


def test_sub_range_of_the_base_set(hip, group16):
    """commit_range of upload_commit_batch (rows [lo, hi) of every column against bases [0, hi - lo)) and a batch at a non-zero base offset:
    the offset enters the payloads next to the shifted pointers"""
    from ezkl_amd import backend as B
    n, lo, hi = 1000, 137, 990
    pts, bases, cols, devs, _ = _set(n)
    pick = [0, 1, 2]                                          # uniform, witness-like, constant
    _, commits = B.upload_commit_batch(bases, [cols[j] for j in pick], commit_range=(lo, hi))
    for i, j in enumerate(pick):
        assert (commits[i] == ob.msm(cols[j][lo:hi], pts[: hi - lo])).all(), j
    m, off = 600, 333                                         # the first m rows of each column against bases [off, off + m)
    got = B.msm_g1_batch_dev(bases, [devs[j].ptr for j in pick], m, offset=off)
    for i, j in enumerate(pick):
        assert (got[i] == ob.msm(cols[j][:m], pts[off: off + m])).all(), j


def test_oversized_partitions_and_heavy_buckets_inside_a_group(hip, group16):
    """2^14 scalars drawn from 1 / 2 / 3 / 7 values (tests/test_gpu_msm.py: test_constant_runs_full_size builds such columns): the pairs of a
    window fall into that many buckets, so the multi-workgroup sort of oversized partitions and the heavy-bucket folds run at blockIdx.z > 0"""
    from ezkl_amd import backend as B
    n = 1 << 14
    rng = np.random.default_rng(14)
    pts = ob.gen_bases(SEED + 12, n)
    bases = B.Bases(pts)
    cols = []
    for distinct in (1, 2, 3, 7):
        vals = rand_fr(rng, distinct)
        runs = np.sort(rng.integers(0, distinct, n)) if distinct != 7 else rng.integers(0, distinct, n)     # long runs, or interleaved
        cols.append(vals[runs])
    devs = [B.DeviceBuffer.from_numpy(c) for c in cols]
    got = B.msm_g1_batch_dev(bases, [d.ptr for d in devs], n)
    for j, c in enumerate(cols):
        assert (got[j] == ob.msm(c, pts)).all(), j
    got = B.msm_g1_batch_dev(bases, [d.ptr for d in reversed(devs)], n)
    for j, c in enumerate(reversed(cols)):
        assert (got[j] == ob.msm(c, pts)).all(), j
    bases.free()
