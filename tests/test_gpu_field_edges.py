"""The production Fr kernels on the edge words of tests/field_edge_ref.py: E(r) holds the residues with a limb of 0 or 0xffffffff and
the pairs whose sum is r - 1, r, r + 1 and whose difference is -1, 0, 1 -- the operands at which a wrong carry, borrow or conditional
subtraction shows, and which uniformly random residues (the rest of the suite) meet with probability 2^-32 per limb.

Expectations are Python integers on the STORED words (Montgomery form, R = 2^256): the stored product of a and b is a b / R mod r, the
stored inverse of a is R^2 / a, the stored one is R mod r.  Sizes cross one structural boundary each and no more."""
import numpy as np
import pytest

import field_edge_ref as F

pytestmark = pytest.mark.gpu

P = F.FR
E = F.edge_words(P)
RINV = pow(F.R256, -1, P)
ONE = F.R256 % P
SCALARS = (0, 1, P - 1, ONE, 1 << 224)


def mm(a, b):
    return a * b * RINV % P


def arr(xs):
    """stored words -> (n, 4) uint64"""
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), np.uint64).reshape(len(xs), 4).copy()


def ints(a):
    raw = np.ascontiguousarray(a, np.uint64).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def cyc(n, start=0, stride=1, words=E):
    return [words[(start + stride * i) % len(words)] for i in range(n)]


def same(got, want, what):
    got = ints(got)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert len(got) == len(want) and not bad, "%s: %d of %d differ; first at %d: got %064x, expected %064x" % (
        what, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]])


@pytest.fixture(scope="module")
def B(hip):
    from ezkl_amd import backend
    return backend


RULES = {"add": lambda a, b: (a + b) % P, "sub": lambda a, b: (a - b) % P, "mul": mm}


@pytest.mark.parametrize("op", ["add", "sub", "mul"])
def test_vec_op_all_pairs_and_aliasing(B, op):
    xs = [a for a in E for _ in E]
    ys = [b for _ in E for b in E]
    n, rule = len(xs), RULES[op]
    da, db, do = (B.DeviceBuffer.from_numpy(arr(xs)), B.DeviceBuffer.from_numpy(arr(ys)), B.DeviceBuffer(32 * n))
    B.vec_op(op, da.ptr, db.ptr, do.ptr, n)
    same(do.to_numpy(), [rule(a, b) for a, b in zip(xs, ys)], op)
    same(da.to_numpy(), xs, op + ": operand a after an out-of-place call")
    B.vec_op(op, da.ptr, db.ptr, da.ptr, n)                               # out == a
    same(da.to_numpy(), [rule(a, b) for a, b in zip(xs, ys)], op + " with out == a")
    B.memcpy_h2d(da.ptr, arr(xs))
    B.vec_op(op, da.ptr, db.ptr, db.ptr, n)                               # out == b
    same(db.to_numpy(), [rule(a, b) for a, b in zip(xs, ys)], op + " with out == b")
    B.vec_op(op, da.ptr, da.ptr, da.ptr, n)                               # a == b == out
    same(da.to_numpy(), [rule(a, a) for a in xs], op + " with a == b == out")
    for d in (da, db, do):
        d.free()


def test_vec_scale(B):
    xs = list(E)
    da, do = B.DeviceBuffer.from_numpy(arr(xs)), B.DeviceBuffer(32 * len(xs))
    for s in SCALARS:
        B.vec_scale(da.ptr, arr([s])[0], do.ptr, len(xs))
        same(do.to_numpy(), [mm(a, s) for a in xs], "vec_scale by %x" % s)
    B.vec_scale(da.ptr, arr([P - 1])[0], da.ptr, len(xs))                 # in place
    same(da.to_numpy(), [mm(a, P - 1) for a in xs], "vec_scale in place")
    da.free(); do.free()


@pytest.mark.parametrize("n", [1, 255, 257, 4097])
def test_vec_fill(B, n):
    do = B.DeviceBuffer(32 * (n + 1))
    for v in SCALARS + (E if n == 257 else ()):
        B.memcpy_h2d(do.ptr, arr([5] * (n + 1)))
        B.vec_fill(do.ptr, arr([v])[0], n)
        same(do.to_numpy(), [v] * n + [5], "vec_fill(%x, %d), and the word after the end" % (v, n))
    do.free()


def scan_ref(xs, op, exclusive):
    acc, out = (0 if op == "add" else ONE), []
    for x in xs:
        if exclusive:
            out.append(acc)
        acc = (acc + x) % P if op == "add" else mm(acc, x)
        if not exclusive:
            out.append(acc)
    return out


NONZERO = tuple(x for x in E if x)


def scan_sequences(n):
    zero_at_boundary = cyc(n, 3, 5, NONZERO)
    if n > 2047:
        zero_at_boundary[2047] = 0                                        # everything after the first chunk is zero
    return [("add", "p-1, 1", [(P - 1, 1)[i & 1] for i in range(n)]),     # the running sum lands on p at every second step
            ("add", "(p+1)/2, (p-1)/2", [((P + 1) // 2, (P - 1) // 2)[i & 1] for i in range(n)]),
            ("add", "E(r)", cyc(n)),
            ("mul", "E(r) without zero", cyc(n, 0, 1, NONZERO)),
            ("mul", "one zero at 2047", zero_at_boundary)]


@pytest.mark.parametrize("n", [2048, 2049])
def test_prefix_scan(B, n):
    di, do = B.DeviceBuffer(32 * n), B.DeviceBuffer(32 * n)
    for op, what, xs in scan_sequences(n):
        for exclusive in (False, True):
            want = scan_ref(xs, op, exclusive)
            B.memcpy_h2d(di.ptr, arr(xs))
            B.prefix_scan(op, di.ptr, do.ptr, n, exclusive=exclusive)
            same(do.to_numpy(), want, "prefix_scan %s %s exclusive=%s n=%d" % (op, what, exclusive, n))
            B.prefix_scan(op, di.ptr, di.ptr, n, exclusive=exclusive)
            same(di.to_numpy(), want, "prefix_scan in place %s %s exclusive=%s n=%d" % (op, what, exclusive, n))
    di.free(); do.free()


def test_batch_invert(B):
    xs = cyc(4097)
    d = B.DeviceBuffer.from_numpy(arr(xs))
    B.batch_invert(d.ptr, len(xs))
    want = [ONE * ONE * pow(a, -1, P) % P if a else 0 for a in xs]
    assert want[E.index(ONE)] == ONE and want[E.index(P - ONE)] == P - ONE and want[E.index(0)] == 0     # 1 and -1 come back as themselves
    same(d.to_numpy(), want, "batch_invert")
    d.free()


@pytest.mark.parametrize("accumulate", [False, True])
def test_lincomb(B, accumulate):
    n = 4097
    cols = [cyc(n, 0, 1), cyc(n, 11, 7), cyc(n, 29, 13)]
    coeffs = [P - 1, E[9], ONE]
    start = cyc(n, 5, 3)
    bufs = [B.DeviceBuffer.from_numpy(arr(c)) for c in cols]
    do = B.DeviceBuffer.from_numpy(arr(start))
    B.lincomb([b.ptr for b in bufs], arr(coeffs), do.ptr, n, accumulate=accumulate)
    want = [((start[i] if accumulate else 0) + sum(mm(c, col[i]) for c, col in zip(coeffs, cols))) % P for i in range(n)]
    same(do.to_numpy(), want, "lincomb accumulate=%s" % accumulate)
    for b in bufs + [do]:
        b.free()


def poly_ref(cs, x):
    acc = 0
    for c in reversed(cs):
        acc = (mm(acc, x) + c) % P
    return acc


def poly_cases(n):
    """(coefficients, x): x the field values 0, 1, -1 and a fixed 'random' point; for 1 and -1 also a vector whose value there is exactly 0"""
    rnd = 0x1d3f5a7c9e0b2d4f6a8c0e1f3b5d7f9a1c3e5a7b9d0f2e4c6a8b0d1f3e5c7a9b % P
    out = [(cyc(n, 2 * k, 1 + 2 * k), x) for k, x in enumerate((0, ONE, P - ONE, rnd))]
    if n == 2:
        out.append(([E[20], P - E[20]], ONE))                             # (c, -c) at 1
    for x in (ONE, P - ONE):
        cs = cyc(n, 7, 3)
        cs[0] = (cs[0] - poly_ref(cs, x)) % P                             # the constant term takes the whole value away
        assert poly_ref(cs, x) == 0
        out.append((cs, x))
    return out


@pytest.mark.parametrize("n", [1, 2, 33, 8193])
def test_eval_polynomial_and_batch(B, n):
    cases = poly_cases(n)
    bufs = [B.DeviceBuffer.from_numpy(arr(cs)) for cs, _ in cases]
    want = [poly_ref(cs, x) for cs, x in cases]
    for b, (cs, x), w in zip(bufs, cases, want):
        same(B.eval_polynomial(b.ptr, n, arr([x])[0]), [w], "eval_polynomial n=%d x=%x" % (n, x))
    same(B.eval_polynomial_batch([b.ptr for b in bufs], n, arr([x for _, x in cases])), want, "eval_polynomial_batch n=%d" % n)
    for b in bufs:
        b.free()


@pytest.mark.parametrize("z", [0, ONE, P - ONE])
def test_kate_division(B, z):
    n = 2049
    a = cyc(n, 1, 3)
    want = [0] * n
    for i in range(n - 1, 0, -1):
        want[i - 1] = (a[i] + mm(z, want[i])) % P
    da, do = B.DeviceBuffer.from_numpy(arr(a)), B.DeviceBuffer(32 * n)
    B.kate_division(da.ptr, arr([z])[0], do.ptr, n)
    same(do.to_numpy(), want, "kate_division z=%x" % z)
    B.kate_division(da.ptr, arr([z])[0], da.ptr, n)                       # out may alias a
    same(da.to_numpy(), want, "kate_division in place z=%x" % z)
    da.free(); do.free()
