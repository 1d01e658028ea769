"""The fixed-base comb (csrc/g1_fixed.hip: backend.g1_fixed_base, and Bases.from_scalars from G1_FIXED_CROSSOVER scalars on): every row
against the oracle's double-and-add on canonical integers (srs_ref.mul_many), byte for byte.

One scalar column of 1000 rows serves every case as a prefix, laid out by the wave (64) and the workgroup (256) of the shared inversion:
  rows 0 .. 63     edge scalars (row 0 is r - 1)          rows 64 .. 127    zero: a whole wave
  rows 128, 191    zero: first and last lane of a wave      rows 256 .. 511   zero: a whole workgroup
  everywhere else  the rest of the edge scalars, then uniform values; n = 1000 leaves the last workgroup ragged"""
import numpy as np
import pytest
from conftest import R, SEED, fe_to_int, rand_fr
from oracle import binding as ob
import srs_ref as SR

pytestmark = pytest.mark.gpu
ROWS = 1000


def _edge_scalars(c):
    """the edges of the recoding into signed c-bit digits"""
    W, half = -(-254 // c), 1 << (c - 1)
    e = [R - 1, 0, 1, 2, R - 2]
    e.append(3 * (1 << 253) - R)                                             # the top window's addition is a doubling modulo r (g1_fixed.hip)
    e.append((1 << 253) - 1)                                                 # all ones: a carry through every window
    e.append(sum(half << (c * w) for w in range(W - 1)) + (1 << 253))        # every digit 2^(c-1), the recoding's tie; the short top one 2^(top_bits-1)
    e += [1 << (c * w) for w in range(W)] + [(1 << (c * w)) - 1 for w in range(W)]
    rng = np.random.default_rng(c)
    for w in range(W):                                                       # a single non-zero window
        hi = (1 << c) if w < W - 1 else (R >> (c * w)) + 1
        e.append(int(rng.integers(1, hi)) << (c * w))
    assert all(0 <= x < R for x in e)
    return e


@pytest.fixture(scope="module")
def column():
    from ezkl_amd import backend as B
    col = [fe_to_int(v) for v in rand_fr(np.random.default_rng(SEED), ROWS)]
    zero = set(range(64, 128)) | {128, 191} | set(range(256, 512))
    free = [r for r in range(ROWS) if r not in zero]
    edges = _edge_scalars(B.G1_FIXED_C)
    assert len(edges) < len(free)
    for r, x in zip(free, edges):
        col[r] = x
    for r in zero:
        col[r] = 0
    return col


@pytest.fixture(scope="module")
def cases(column):
    """base name -> (point, the 1000 expected records)"""
    other = ob.gen_bases(SEED + 11, 3)[2]
    return {"generator": (SR.G, SR.mul_many(SR.G, column)), "other": (other, SR.mul_many(other, column)),
            "identity": (np.zeros(8, np.uint64), np.zeros((ROWS, 8), np.uint64))}


def _comb(B, P, scalars, n):
    dev, out = B.DeviceBuffer.from_numpy(SR.fes(scalars[:n])), B.DeviceBuffer(64 * n)
    B.g1_fixed_base(P, dev.ptr, n, out.ptr)
    got = out.to_numpy(shape=(n, 8))
    dev.free(); out.free()
    return got


def _bad_rows(got, want):
    return np.flatnonzero((got != want).any(axis=1)).tolist()


@pytest.mark.parametrize("base", ["generator", "other", "identity"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_every_row_matches_double_and_add(hip, column, cases, n, base):
    from ezkl_amd import backend as B
    P, want = cases[base]
    assert not _bad_rows(_comb(B, P, column, n), want[:n])


def test_every_scalar_zero(hip):
    from ezkl_amd import backend as B
    assert not _comb(B, SR.G, [0] * 257, 257).any()


def test_from_scalars_gives_the_same_records_on_both_sides_of_the_crossover(hip, column, cases):
    from ezkl_amd import backend as B
    P, want = cases["generator"]
    for n in (B.G1_FIXED_CROSSOVER - 1, B.G1_FIXED_CROSSOVER):
        rows = np.arange(n) % ROWS
        dev = B.DeviceBuffer.from_numpy(SR.fes([column[r] for r in rows]))
        b = B.Bases.from_scalars(P, dev.ptr, n)
        got = b.download()
        b.free(); dev.free()
        assert not _bad_rows(got, want[rows])


def test_out_is_any_aligned_resident_buffer_and_nothing_around_it_is_written(hip, column, cases):
    from ezkl_amd import backend as B
    n, P, want = 65, *cases["other"]
    guard = np.full(2 + 8 * n + 2, 0xA5A5A5A5A5A5A5A5, np.uint64)             # 16 bytes, n records, 16 bytes
    buf, dev = B.DeviceBuffer.from_numpy(guard), B.DeviceBuffer.from_numpy(SR.fes(column[:n]))
    B.g1_fixed_base(P, dev.ptr, n, buf.ptr + 16)
    got = buf.to_numpy()
    buf.free(); dev.free()
    assert (got[:2] == guard[:2]).all() and (got[-2:] == guard[-2:]).all()
    assert not _bad_rows(got[2:-2].reshape(n, 8), want[:n])


def test_the_region_is_timed(hip, column):
    from ezkl_amd import backend as B
    _comb(B, SR.G, column, 64)
    assert B.last_kernel_ms("fixed_base") > 0
