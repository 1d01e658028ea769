"""The point predicate of an SRS file's reader, restated in Python integers: what ezkl_amd/csrc/srs_check.hpp decides about a 64-byte record
(x then y, 32-byte little-endian Montgomery Fq words) and what ezkl_hip_bases_check reports about a range of them.  Nothing here touches
the device or either library.

    reason 0  valid (the all-zero record is the identity: valid, flagged apart)
           1  x >= q as a 256-bit integer        2  y >= q        3  y^2 != x^3 + 3        -- the first that applies"""
import numpy as np

Q = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
MONT = 1 << 256
RINV = pow(MONT, -1, Q)


def words(p):
    """a record (64 bytes, or 8 x u64) -> the two 256-bit integers it stores"""
    b = p.tobytes() if isinstance(p, np.ndarray) else bytes(p)
    assert len(b) == 64
    return int.from_bytes(b[:32], "little"), int.from_bytes(b[32:], "little")


def record(xw, yw):
    """two stored 256-bit integers -> 8 x u64"""
    return np.frombuffer(xw.to_bytes(32, "little") + yw.to_bytes(32, "little"), np.uint64).copy()


def affine(x, y):
    """a point given by canonical coordinates -> its record"""
    return record(x * MONT % Q, y * MONT % Q)


def reason(p):
    """-> (reason code, is the identity)"""
    xw, yw = words(p)
    if xw == 0 and yw == 0:
        return 0, True
    if xw >= Q:
        return 1, False
    if yw >= Q:
        return 2, False
    x, y = xw * RINV % Q, yw * RINV % Q
    return (0 if (y * y - x * x * x - 3) % Q == 0 else 3), False


def check(points, first=0, n=None):
    """Bases.check of points[first : first + n], by the definition: indices are those of the whole set"""
    n = len(points) - first if n is None else n
    bad, ids, first_bad, why = 0, 0, None, 0
    for i in range(first, first + n):
        r, ident = reason(points[i])
        ids += ident
        if r:
            bad += 1
            if first_bad is None:
                first_bad, why = i, r
    return dict(bad=bad, first_bad=first_bad, reason=why, identities=ids)


def sqrt(a):
    """a square root of a mod q (q = 3 mod 4), or None"""
    y = pow(a % Q, (Q + 1) // 4, Q)
    return y if y * y % Q == a % Q else None


def double(x, y):
    """2 (x, y) on y^2 = x^3 + 3, canonical coordinates, y != 0"""
    lam = 3 * x * x * pow(2 * y, -1, Q) % Q
    x2 = (lam * lam - 2 * x) % Q
    return x2, (lam * (x - x2) - y) % Q


def bad_point(why, salt=0):
    """a record the predicate refuses for reason `why` and no earlier one (salt varies it)"""
    if why == 1:
        return record(Q + salt, 2 * MONT % Q)
    if why == 2:
        return record(MONT % Q, Q + salt)
    x = 5 + salt
    while sqrt(x ** 3 + 3) is not None:                  # an x with no y at all: whatever y, the equation fails
        x += 1
    return affine(x, 7)
