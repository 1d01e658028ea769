"""Input columns for the NTT tests (tests/test_gpu_ntt_plans.py and the child processes it starts): random residues with the words at
which a lazily reduced 256-bit input goes wrong scattered among them.  No GPU and no oracle here."""
import numpy as np

from conftest import R, rand_fr
from field_edge_ref import edge_words

# the words of test_gpu_ntt.test_words_that_are_not_canonical: at and above the modulus, the all-ones word, the ends of the canonical range
SPECIAL = [(1 << 256) - 1, R, R + 5, 2 * R - 1, 5 * R + 12345, (1 << 256) - R, 0, R - 1]
STRIDE = 7919                                # prime: coprime to 3 and to every tile width


def words(values):
    return np.array([[(v >> (64 * q)) & 0xFFFFFFFFFFFFFFFF for q in range(4)] for v in values], np.uint64).reshape(len(values), 4)


def edge_column(rng, n):
    """(raw, reduced): n random residues, with SPECIAL and field_edge_ref.edge_words scattered at stride 7919 from element 0 on, and the
    all-ones word, the modulus and 2p - 1 on each of the three classes of index mod 3 at the very end and just behind the start.  `raw` is
    what the device gets (256-bit words), `reduced` the same column with every word reduced modulo the modulus: what the oracle gets."""
    raw = rand_fr(rng, n)
    values = (SPECIAL + list(edge_words(R)))[:max(1, n // 4)]
    at = {(j * STRIDE) % n: v for j, v in enumerate(values)}
    if n >= 64:
        for q in range(3):
            at[n - 1 - q] = (1 << 256) - 1               # last rows of the last tile
            at[n - 4 - q] = 2 * R - 1
            at[3 + q] = R                                # first row of the first tile (element 0 holds SPECIAL[0])
    pos = sorted(at)
    red = raw.copy()
    raw[pos] = words([at[i] for i in pos])
    red[pos] = words([at[i] % R for i in pos])
    if n >= 64:
        big = {i % 3 for i in pos if at[i] >= R}
        assert big == {0, 1, 2}                          # words at or above the modulus on every class of index mod 3
    return raw, red


def to_coset_major(nat, k, ek):
    """natural-order extended column -> coset-major: cm[b 2^k + j] = nat[E j + b]"""
    E = 1 << (ek - k)
    return np.ascontiguousarray(nat.reshape(1 << k, E, 4).transpose(1, 0, 2)).reshape(1 << ek, 4)


def sentinel(count, salt=0):
    """`count` distinct words no transform of these tests produces by accident"""
    i = np.arange(count, dtype=np.uint64) + np.uint64(salt)
    return np.stack([i * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1), ~i, i ^ np.uint64(0xA5A5A5A5A5A5A5A5), np.full(count, 0xDEADBEEFDEADBEEF, np.uint64)], axis=1)
