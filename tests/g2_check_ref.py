"""What ezkl_hip_g2_check_dev decides about 128-byte G2 records (x.c0, x.c1, y.c0, y.c1: 32-byte little-endian Montgomery Fq words),
restated in Python integers.  Nothing here touches the device or the library.  A point is None (the identity) or ((x0, x1), (y0, y1)).

    reason 0  valid (the all-zero record is the identity: valid, counted apart)
           1  a coordinate word >= q        2  y^2 != x^3 + 3 / xi        3  on the twist, [r]P != O        -- the first that applies"""
import os

import numpy as np

Q = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
X = 4965661367192848881                                       # the BN parameter: q = 36x^4 + 36x^3 + 24x^2 + 6x + 1
MONT = 1 << 256
RINV = pow(MONT, -1, Q)
XI = (9, 1)
WORDS = {0: None, 1: "coordinate not below the field modulus", 2: "point not on the curve", 3: "point not in the subgroup"}


def f2_add(a, b): return ((a[0] + b[0]) % Q, (a[1] + b[1]) % Q)
def f2_sub(a, b): return ((a[0] - b[0]) % Q, (a[1] - b[1]) % Q)
def f2_mul(a, b): return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)
def f2_conj(a): return (a[0], -a[1] % Q)


def f2_inv(a):
    n = pow(a[0] * a[0] + a[1] * a[1], -1, Q)
    return (a[0] * n % Q, -a[1] * n % Q)


def f2_pow(a, e):
    acc = (1, 0)
    while e:
        if e & 1:
            acc = f2_mul(acc, a)
        a, e = f2_mul(a, a), e >> 1
    return acc


B2 = f2_mul((3, 0), f2_inv(XI))                                # the twist: y^2 = x^3 + 3 / xi
PSI_X, PSI_Y = f2_pow(XI, (Q - 1) // 3), f2_pow(XI, (Q - 1) // 2)


def _sqrt(a):
    y = pow(a, (Q + 1) // 4, Q)
    return y if y * y % Q == a % Q else None


def f2_sqrt(a):
    """a square root of a in Fq2 or None: with s^2 = a0^2 + a1^2, c0^2 = (a0 +- s) / 2 and c1 = a1 / (2 c0)"""
    if a[1] % Q == 0:
        y = _sqrt(a[0])
        if y is not None:
            return (y, 0)
        y = _sqrt(-a[0] % Q)
        return None if y is None else (0, y)
    s = _sqrt((a[0] * a[0] + a[1] * a[1]) % Q)
    if s is None:
        return None
    for t in (s, -s):
        c0 = _sqrt((a[0] + t) * pow(2, -1, Q) % Q)
        if c0:
            c = (c0, a[1] * pow(2 * c0, -1, Q) % Q)
            return c if f2_mul(c, c) == (a[0] % Q, a[1] % Q) else None
    return None


def on_curve(p):
    return p is None or f2_mul(p[1], p[1]) == f2_add(f2_mul(f2_mul(p[0], p[0]), p[0]), B2)


def neg(p):
    return None if p is None else (p[0], f2_sub((0, 0), p[1]))


def add(p, q):
    if p is None or q is None:
        return q if p is None else p
    if p[0] == q[0]:
        if p[1] != q[1] or p[1] == (0, 0):
            return None
        lam = f2_mul(f2_mul((3, 0), f2_mul(p[0], p[0])), f2_inv(f2_add(p[1], p[1])))
    else:
        lam = f2_mul(f2_sub(q[1], p[1]), f2_inv(f2_sub(q[0], p[0])))
    x = f2_sub(f2_sub(f2_mul(lam, lam), p[0]), q[0])
    return (x, f2_sub(f2_mul(lam, f2_sub(p[0], x)), p[1]))


def mul(p, k):
    acc = None
    for bit in bin(k)[2:]:
        acc = add(acc, acc)
        if bit == "1":
            acc = add(acc, p)
    return acc


def in_subgroup(p):
    """the definition: [r]P == O, by double-and-add"""
    return mul(p, R) is None


def psi(p):
    return None if p is None else (f2_mul(f2_conj(p[0]), PSI_X), f2_mul(f2_conj(p[1]), PSI_Y))


def endo_test(p):
    """[x+1]P + psi([x]P) + psi^2([x]P) == psi^3([2x]P): the kernel's test"""
    a = mul(p, X)
    return add(add(add(a, p), psi(a)), psi(psi(a))) == psi(psi(psi(add(a, a))))


def encode(p):
    if p is None:
        return np.zeros(16, np.uint64)
    return np.frombuffer(b"".join((c * MONT % Q).to_bytes(32, "little") for c in (*p[0], *p[1])), np.uint64).copy()


def decode(rec):
    """a record -> (the four stored 256-bit words, the point they stand for when all are below q)"""
    b = np.ascontiguousarray(rec, np.uint64).tobytes()
    w = [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(4)]
    c = [v * RINV % Q for v in w]
    return w, (None if not any(w) else ((c[0], c[1]), (c[2], c[3])))


def reason(rec):
    """-> (reason code, is the identity)"""
    w, p = decode(rec)
    if p is None:
        return 0, True
    if any(v >= Q for v in w):
        return 1, False
    if not on_curve(p):
        return 2, False
    return (0 if in_subgroup(p) else 3), False


def classify(points, known_good=()):
    """the four words of ezkl_hip_g2_check_dev: {bad, index, reason, identities}; rows listed in known_good are [s]g2 by construction and
    are not put through [r]P again"""
    bad, ids, index, why = 0, 0, None, None
    for i, rec in enumerate(points):
        r, ident = (0, False) if i in known_good else reason(rec)
        ids += ident
        if r:
            bad += 1
            if index is None:
                index, why = i, WORDS[r]
    return dict(bad=bad, index=index, reason=why, identities=ids)


def generator():
    """g2 of the golden k = 6 SRS file"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kzg_k6.srs")
    raw = open(path, "rb").read()
    return decode(np.frombuffer(raw[-256:-128], np.uint64))[1]


def good_points(n):
    """[1]g2 .. [n]g2"""
    g, out = generator(), []
    for _ in range(n):
        out.append(add(out[-1], g) if out else g)
    return out


def twist_points(n, start=1):
    """n points of the twist from successive x = (i, 1), i >= start: on the curve, and (the cofactor is about 2^254) not of order r --
    which the caller asserts with in_subgroup"""
    out, i = [], start
    while len(out) < n:
        x = (i, 1)
        y = f2_sqrt(f2_add(f2_mul(f2_mul(x, x), x), B2))
        if y is not None:
            out.append((x, y))
        i += 1
    return out


def bad_record(why, salt=0):
    """a record refused for reason `why` and no earlier one"""
    if why == 1:
        rec = encode(good_points(1)[0])
        rec[4 * (salt % 4):4 * (salt % 4) + 4] = np.frombuffer((Q + salt).to_bytes(32, "little"), np.uint64)
        return rec
    if why == 2:
        p = twist_points(1, 1 + salt)[0]
        return encode((p[0], f2_add(p[1], (1, 0))))
    return encode(twist_points(1, 1 + salt)[0])
