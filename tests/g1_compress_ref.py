"""Compressed G1 points in Python integers: the reference of ezkl_amd/csrc/g1_compress.hip.  The encoding is restated from
ezkl_amd/csrc/g1_encoding.hpp: x canonical little-endian, bit 254 the parity of the canonical y, bit 255 the identity flag.
Reasons: 0 valid, 1 x >= q, 3 x^3 + 3 is not a square, 4 malformed flags.  Nothing here touches the device or either library."""
import numpy as np

from srs_check_ref import Q, RINV, affine, double, words

SIGN_BIT, IDENTITY_BIT = 254, 255
IDENTITY = (1 << IDENTITY_BIT).to_bytes(32, "little")


def compress(rec):
    """a 64-byte record (Montgomery x, y; all zero = the identity) -> 32 bytes"""
    xw, yw = words(rec)
    if xw == 0 and yw == 0:
        return IDENTITY
    return ((xw * RINV % Q) | ((yw * RINV % Q & 1) << SIGN_BIT)).to_bytes(32, "little")


def decompress(b):
    """32 bytes -> (record as 8 x u64 or None, reason)"""
    v = int.from_bytes(bytes(b), "little")
    sign, ident, x = (v >> SIGN_BIT) & 1, v >> IDENTITY_BIT, v & ((1 << SIGN_BIT) - 1)
    if ident:
        return (None, 4) if x or sign else (np.zeros(8, np.uint64), 0)
    if x >= Q:
        return None, 1
    t = (x * x * x + 3) % Q
    y = pow(t, (Q + 1) // 4, Q)
    if y * y % Q != t:
        return None, 3
    return affine(x, y if (y & 1) == sign or y == 0 else Q - y), 0


def add(p, q):
    """affine addition of two distinct points with distinct x"""
    lam = (q[1] - p[1]) * pow(q[0] - p[0], -1, Q) % Q
    x = (lam * lam - p[0] - q[0]) % Q
    return x, (lam * (p[0] - x) - p[1]) % Q


def mul(k, p):
    acc = None
    for bit in bin(k)[2:]:
        acc = double(*acc) if acc else None
        if bit == "1":
            acc = add(acc, p) if acc else p
    return acc


def multiples(n, seed):
    """n multiples of the generator as records: (a + i d) G for two seeded 64-bit a, d"""
    a, d = (int(v) | 1 << 63 for v in np.random.default_rng(seed).integers(0, 1 << 63, 2))
    p, step, out = mul(a, (1, 2)), mul(d, (1, 2)), []
    for _ in range(n):
        out.append(affine(*p))
        p = add(p, step)
    return np.array(out)
