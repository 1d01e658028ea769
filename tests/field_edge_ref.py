"""Operands and expected words for the field-primitive probe (ezkl_hip_field_probe_dev, csrc/fieldprobe.hip) and for the host halves of
Field<P> (tests/cpp/field_host_probe.cpp), in plain Python integers.  Nothing here calls the C oracle or the library: a mistake shared
with either could hide.

A carry, a borrow or a conditional subtraction goes wrong at a limb that is exactly 0, 0xffffffff or 2^29 - 1, or at a value exactly
on p, 2p or K p; uniformly random residues meet such a case with probability 2^-29 .. 2^-32 per limb.  So the operand lists below are
built from those words, deterministically, and the random rows that follow them are only there for the bulk.

Every case is (operands, expected, n_edge): one uint32 array (n, words) per operand, the expected result rows, and how many of the
leading rows are edge rows (the rest are random).  Every operand respects the precondition its header states; check_domain() of a case
asserts it and tests/test_field_edge_ref.py runs it for all of them.
"""
import functools
import random

import numpy as np

FR = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
FQ = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
MODS = {"fr": FR, "fq": FQ, "fr29": FR, "fq29": FQ}
R256 = 1 << 256
R261 = 1 << 261
M29 = (1 << 29) - 1
M32 = (1 << 32) - 1
N_RANDOM = 4096
LIVE_ROWS, LIVE_SALT = 6, 64                    # csrc/fieldprobe.hip


# ---------------------------------------------------------------------------------------------------------------- words and limbs
def words32(x):
    assert 0 <= x < R256
    return [(x >> (32 * i)) & M32 for i in range(8)]


def from_words32(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


def limbs29(x):
    """limbs 0..7 of 29 bits each, limb 8 = x >> 232"""
    assert 0 <= x and (x >> 232) <= M32
    return [(x >> (29 * i)) & M29 for i in range(8)] + [x >> 232]


def value29(v):
    return sum(int(x) << (29 * i) for i, x in enumerate(v))


def redc(T, p, bits):
    """(T + ((T mod 2^bits) N' mod 2^bits) p) / 2^bits with N' = -p^-1 mod 2^bits: the one value every digit-serial form must produce"""
    B = 1 << bits
    m = (T % B) * (-pow(p, -1, B) % B) % B
    t = T + m * p
    assert t % B == 0
    return t >> bits


def subc(p, KI):
    """K p (K = 2 << KI) with 2^29 lent from every limb to the one below: field29.hpp's subtraction constant, restated"""
    k = limbs29((2 << KI) * p)
    c = [k[0] + (1 << 29)] + [k[i] + (1 << 29) - 1 for i in range(1, 8)] + [k[8] - 1]
    assert value29(c) == (2 << KI) * p
    return c


def _uniq(xs):
    seen, out = set(), []
    for x in xs:
        if x not in seen:
            seen.add(x)
            out.append(x)
    return out


# ---------------------------------------------------------------------------------------------------------------- radix 2^32 operands
@functools.lru_cache(None)
def edge_words(p):
    """E(p): canonical words (< p) at which a limb is 0 or all ones, or a sum / difference lands on p - 1, p, p + 1 or -1, 0, 1"""
    pw = words32(p)
    r1 = R256 % p
    e = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2]
    for i in range(1, 8):
        e += [(1 << (32 * i)) - 1, 1 << (32 * i), (1 << (32 * i)) + 1]
    e += [(1 << 253) - 1, 1 << 253]
    e += [p - (1 << (32 * i)) for i in range(1, 8)]
    e += [M32 << (32 * i) for i in range(7)]                         # the one in limb 7 is >= p: it is in any_words() only
    e += [((1 << 224) - 1) + ((pw[7] - 1) << 224)]
    e += [pw[i] << (32 * i) for i in range(8)]
    e += [pw[i] for i in range(8)]                                   # pw[0] times the stored word 1: the first quotient digit is 0xffffffff
    e += [r1, r1 * r1 % p, p - r1]
    e = _uniq(e)
    assert all(0 <= x < p for x in e)
    return tuple(e)


def lazy_words(p, bound):
    """E(p) and the values around p, 2p, 4p and 2^256 that a lazily reduced operand may take, as far as they are below `bound`"""
    extra = [p, p + 1, 2 * p - 1, 2 * p, 2 * p + 1, 4 * p - 1, R256 - 1, R256 - p, M32 << 224]
    return tuple(_uniq(list(edge_words(p)) + [x for x in extra if x < bound]))


def any_words(p):
    return lazy_words(p, R256)


def _rng(tag):
    return random.Random("field-edges/" + tag)


def _pairs(xs, ys, rng, bx, by):
    return [(x, y) for x in xs for y in ys], [(rng.randrange(bx), rng.randrange(by)) for _ in range(N_RANDOM)]


def _singles(xs, rng, bound):
    return [(x,) for x in xs], [(rng.randrange(bound),) for _ in range(N_RANDOM)]


def reduce_once_rule(a, p):
    return a - p if a >= p else a


# name -> (operand bounds as multiples of p (None: any 256-bit word), expected(p, *operands), rows(p, rng) -> (edge rows, random rows))
def _table32():
    def canon2(p, rng): return _pairs(edge_words(p), edge_words(p), rng, p, p)
    def canon1(p, rng): return _singles(edge_words(p), rng, p)
    def lazy2(p, rng): return _pairs(lazy_words(p, 2 * p), lazy_words(p, 2 * p), rng, 2 * p, 2 * p)
    rinv = lambda p: pow(R256, -1, p)
    return {
        "add": ((1, 1), lambda p, a, b: (a + b) % p, canon2),
        "sub": ((1, 1), lambda p, a, b: (a - b) % p, canon2),
        "neg": ((1,), lambda p, a: -a % p, canon1),
        "dbl": ((1,), lambda p, a: 2 * a % p, canon1),
        "reduce_once": ((2,), lambda p, a: reduce_once_rule(a, p), lambda p, rng: _singles(lazy_words(p, 2 * p), rng, 2 * p)),
        "mul": ((1, 1), lambda p, a, b: a * b * rinv(p) % p, canon2),
        "mul_inl": ((1, 1), lambda p, a, b: a * b * rinv(p) % p, canon2),
        "sqr": ((1,), lambda p, a: a * a * rinv(p) % p, canon1),
        # the DEVICE half: no final subtraction, the result is the Montgomery reduction itself and must be below 2p
        "mul_lazy": ((4, 1), lambda p, a, b: redc(a * b, p, 256), lambda p, rng: _pairs(lazy_words(p, 4 * p), edge_words(p), rng, 4 * p, p)),
        "redc": ((None,), lambda p, a: a * rinv(p) % p, lambda p, rng: _singles(any_words(p), rng, R256)),
        "from_mont": ((1,), lambda p, a: a * rinv(p) % p, canon1),
        "to_mont": ((1,), lambda p, a: a * R256 % p, canon1),
        "add_lazy": ((2, 2), lambda p, a, b: a + b - 2 * p if a + b >= 2 * p else a + b, lazy2),
        "sub_lazy": ((2, 2), lambda p, a, b: a - b + 2 * p, lazy2),
        "reduce_2p": ((4,), lambda p, a: a - 2 * p if a >= 2 * p else a, lambda p, rng: _singles(lazy_words(p, 4 * p), rng, 4 * p)),
        # Fermat, 255 products per row: the edge list only
        "inv": ((1,), lambda p, a: R256 * R256 * pow(a, -1, p) % p if a else 0, lambda p, rng: ([(x,) for x in edge_words(p)], [])),
    }


TABLE32 = _table32()


def host_expected32(prim, p, *ops):
    """what the __host__ halves of Field<P> return: as the device, except that mul_lazy's host half returns the canonical residue"""
    if prim == "mul_lazy":
        return ops[0] * ops[1] * pow(R256, -1, p) % p
    return TABLE32[prim][1](p, *ops)


@functools.lru_cache(None)
def rows32(field, prim):
    """(edge rows, random rows) of operand tuples, Python integers"""
    p = MODS[field]
    edge, rnd = TABLE32[prim][2](p, _rng("%s.%s" % (field, prim)))
    return edge, rnd


def _arr(rows, width):
    return np.array(rows, dtype=np.uint32).reshape(len(rows), width)


# ---------------------------------------------------------------------------------------------------------------- radix 2^29 operands
def loose_limbs(rng, mod, vmax_p, units):
    """as tests/test_montmul29_asm.py: a value < vmax_p * mod written with limbs below units * 2^29 (limb 8 holds the rest)"""
    x = rng.randrange(vmax_p * mod)
    v = limbs29(x)
    for i in range(8):
        k = min(rng.randrange(units), v[i + 1])
        if k:
            v[i + 1] -= k
            v[i] += k << 29
    assert value29(v) == x and all(l < units << 29 for l in v[:8])
    return v


def class_max(p, units, top):
    """limbs 0..7 at the maximum of the class, units * 2^29 - 1; limb 8 is 0, or (top) the largest that keeps the value below 32 p"""
    low = value29([(units << 29) - 1] * 8 + [0])
    return [(units << 29) - 1] * 8 + [(32 * p - 1 - low) >> 232 if top else 0]


@functools.lru_cache(None)
def values29(p):
    """normalized values in [0, 2^261): every radix-2^32 edge word, every multiple of p and its neighbours, the powers of the limb base"""
    v = list(any_words(p))
    for j in range(R261 // p + 1):
        v += [j * p - 1, j * p, j * p + 1]
    v.append(R261 - 1)
    for i in range(9):
        v += [(1 << (29 * i)) - 1, 1 << (29 * i), M29 << (29 * i)]
    return tuple(_uniq(x for x in v if 0 <= x < R261))


def _product_rows(p, rng, pairings):
    """pairings: tuples of limb classes per operand.  Edge rows: every operand at its class maximum with limb 8 at 0 and at its top, the
    normalized edge values below 32 p among themselves; random rows: loose operands of the pairings in turn"""
    edge = []
    for cls in pairings:
        for tops in range(1 << len(cls)):
            edge.append(tuple(tuple(class_max(p, u, (tops >> k) & 1)) for k, u in enumerate(cls)))
    small = [tuple(limbs29(x)) for x in values29(p) if x < 32 * p]
    arity = len(pairings[0])
    for stride in (0, 1, 7):
        for i in range(len(small)):
            edge.append(tuple(small[(i + stride * (k + 1) * (k > 0)) % len(small)] for k in range(arity)))
    edge = _uniq(edge)
    rnd = []
    for i in range(N_RANDOM):
        cls = pairings[i % len(pairings)]
        rnd.append(tuple(tuple(loose_limbs(rng, p, 32, u)) for u in cls))
    return edge, rnd


MUL_PAIRINGS = ((1, 1), (3, 1), (2, 3))
SQR_CLASSES = ((1,), (2,))
MUL2ADD_PAIRINGS = ((1, 3, 2, 1),)


def _sub_rows(p, KI, rng, with_a):
    K = 2 << KI
    top = ((K - 1) * p >> 232) - 1
    bs = [[0] * 9, limbs29((K - 1) * p - 1), [M29] * 8 + [0], [M29] * 8 + [top]]
    bs += [limbs29(rng.randrange((K - 1) * p)) for _ in range(60)]
    if not with_a:
        return [(tuple(b),) for b in bs], []
    As = [[0] * 9, class_max(p, 3, 0), class_max(p, 3, 1), class_max(p, 1, 1), limbs29(p - 1)] + [loose_limbs(rng, p, 32, 3) for _ in range(11)]
    return [(tuple(a), tuple(b)) for a in As for b in bs], []


def _is_zero_rows(p):
    v = []
    for j in range(32):
        v += [j * p - 1, j * p, j * p + 1]
        v += [j * p + (t << 29) for t in (1, 2, M29, 1 << 28, (1 << 200) + 1)]       # the low limb is that of j p: only the full compare tells
    v += list(values29(p))
    return [(tuple(limbs29(x)),) for x in _uniq(v) if 0 <= x < 32 * p], []


def _table29():
    t = {}

    def add(name, arity, w_in, w_out, expected, rows, fq_only=False):
        t[name] = (arity, w_in, w_out, expected, rows, fq_only)

    def words_rows(p, rng):
        ws = _uniq(list(any_words(FR)) + list(any_words(FQ)))
        return [(tuple(words32(x)),) for x in ws], [(tuple(words32(rng.randrange(R256))),) for _ in range(N_RANDOM)]

    def limbs_rows(p, rng):
        e, r = words_rows(p, rng)
        return [(tuple(limbs29(from_words32(w))),) for (w,) in e], [(tuple(limbs29(from_words32(w))),) for (w,) in r]

    def normalize_rows(p, rng):
        e = [(tuple(limbs29(x)),) for x in values29(p)]
        e += [(tuple(class_max(p, u, top)),) for u in (1, 2, 3) for top in (0, 1)]
        e += [((0xfffffff7,) * 9,), ((0xfffffff7,) * 8 + (0,),), ((M29,) * 9,), ((M29 + 1,) * 9,)]      # limbs < 2^32 - 2^3 on entry
        return e, [(tuple(loose_limbs(rng, p, 32, 1 + i % 3)),) for i in range(N_RANDOM)]

    def norm_values(p, rng): return [(tuple(limbs29(x)),) for x in values29(p)], [(tuple(limbs29(rng.randrange(R261))),) for _ in range(N_RANDOM)]
    prod = lambda p, *ops: limbs29(redc(value29(ops[0]) * value29(ops[1]), p, 261))
    square = lambda p, a: limbs29(redc(value29(a) ** 2, p, 261))
    add("unpack", 1, 8, 9, lambda p, w: limbs29(from_words32(w)), words_rows)
    add("pack", 1, 9, 8, lambda p, v: words32(value29(v)), limbs_rows)                    # pack(unpack(w)) = w
    add("normalize", 1, 9, 9, lambda p, v: limbs29(value29(v)), normalize_rows)
    add("mul", 2, 9, 9, prod, lambda p, rng: _product_rows(p, rng, MUL_PAIRINGS))
    add("mul_cold", 2, 9, 9, prod, lambda p, rng: _product_rows(p, rng, MUL_PAIRINGS))
    add("sqr", 1, 9, 9, square, lambda p, rng: _product_rows(p, rng, SQR_CLASSES))
    add("sqr_cold", 1, 9, 9, square, lambda p, rng: _product_rows(p, rng, SQR_CLASSES))
    add("mul2add", 4, 9, 9, lambda p, a, b, c, d: limbs29(redc(value29(a) * value29(b) + value29(c) * value29(d), p, 261)),
        lambda p, rng: _product_rows(p, rng, MUL2ADD_PAIRINGS), fq_only=True)
    for KI in range(7):
        add("sub%d" % KI, 2, 9, 9, lambda p, a, b, KI=KI: [x + c - y for x, c, y in zip(a, subc(p, KI), b)], lambda p, rng, KI=KI: _sub_rows(p, KI, rng, True))
        add("neg%d" % KI, 1, 9, 9, lambda p, b, KI=KI: [c - y for c, y in zip(subc(p, KI), b)], lambda p, rng, KI=KI: _sub_rows(p, KI, rng, False))
    for KI in range(4):
        add("cond_sub%d" % KI, 1, 9, 9, lambda p, v, KI=KI: limbs29(value29(v) - (p << KI) if value29(v) >= (p << KI) else value29(v)), norm_values)
    add("canonical", 1, 9, 9, lambda p, v: limbs29(value29(v) % p), norm_values)
    add("is_zero_mod_p", 1, 9, 1, lambda p, v: [1 if value29(v) % p == 0 else 0], lambda p, rng: _is_zero_rows(p))
    return t


TABLE29 = _table29()


@functools.lru_cache(None)
def rows29(field, prim):
    prim = {"mul_cold": "mul", "sqr_cold": "sqr"}.get(prim, prim)          # the out-of-line forms get the very rows of the inline ones
    return TABLE29[prim][4](MODS[field], _rng("%s.%s" % (field, prim)))


# ---------------------------------------------------------------------------------------------------------------- live-register probes
# name -> (base primitive whose rule gives the product, rows taken from the base's lists)
LIVE = {
    "fr.live_mul_inl": "fr.mul_inl", "fq.live_mul_inl": "fq.mul_inl",
    "fr.live_mul_lazy": "fr.mul_lazy", "fq.live_mul_lazy": "fq.mul_lazy",
    "fr.live_mul_single": "fr.mul_lazy", "fq.live_mul_single": "fq.mul_lazy",          # mont_mul_asm1_* itself: the same rule
    "fr29.live_mul": "fr29.mul", "fq29.live_mul": "fq29.mul",
    "fr29.live_sqr": "fr29.sqr", "fq29.live_sqr": "fq29.sqr",
    "fq29.live_mul2add": "fq29.mul2add",
}
LIVE_N = 389                                   # two blocks of 256, the second one ragged


def live_salt():
    return [0x9e3779b9 * (j + 1) & M32 for j in range(LIVE_SALT)]


# ---------------------------------------------------------------------------------------------------------------- cases
def names():
    """every name the probe must know"""
    out = ["%s.%s" % (f, prim) for f in ("fr", "fq") for prim in TABLE32]
    out += ["%s.%s" % (f, prim) for f in ("fr29", "fq29") for prim, e in TABLE29.items() if not (e[5] and f != "fq29")]
    return sorted(out + list(LIVE))


def shape(name):
    """(operands, words per operand row, words per result row)"""
    if name in LIVE:
        arity, w_in, _ = shape(LIVE[name])
        return arity, w_in, w_in + LIVE_ROWS * w_in + LIVE_SALT
    field, prim = name.split(".")
    if field in ("fr", "fq"):
        return len(TABLE32[prim][0]), 8, 8
    return TABLE29[prim][:3]


def int_rows(name):
    """(edge rows, random rows): per row a tuple of operands, each a Python integer (radix 2^32) or a tuple of words"""
    field, prim = name.split(".")
    return rows32(field, prim) if field in ("fr", "fq") else rows29(field, prim)


def expected_words(name, ops):
    field, prim = name.split(".")
    p = MODS[field]
    if field in ("fr", "fq"):
        return words32(TABLE32[prim][1](p, *ops))
    return TABLE29[prim][3](p, *ops)


def operand_words(name, x):
    return words32(x) if name.split(".")[0] in ("fr", "fq") else list(x)


@functools.lru_cache(None)
def case(name):
    """(operands, expected, n_edge) as uint32 arrays"""
    if name in LIVE:
        base = LIVE[name]
        edge, rnd = int_rows(base)
        step = max(1, len(edge) // (LIVE_N // 2))
        rows = (edge[::step] + rnd)[:LIVE_N]           # edge rows first, filled up with random ones
        assert len(rows) == LIVE_N
        arity, w_in, w_out = shape(name)
        ops = [_arr([operand_words(base, r[k]) for r in rows], w_in) for k in range(arity)]
        exp = []
        for i, r in enumerate(rows):
            row = list(expected_words(base, r))
            for k in range(LIVE_ROWS):
                row += [int(x) for x in ops[0][(i + 1 + k) % LIVE_N]]
            exp.append(row + live_salt())
        return ops, _arr(exp, w_out), min(len(edge[::step]), LIVE_N)
    edge, rnd = int_rows(name)
    rows = edge + rnd
    arity, w_in, w_out = shape(name)
    ops = [_arr([operand_words(name, r[k]) for r in rows], w_in) for k in range(arity)]
    return ops, _arr([expected_words(name, r) for r in rows], w_out), len(edge)


def check_domain(name):
    """the preconditions of field.hpp / field29.hpp on every row of the case"""
    base = LIVE.get(name, name)
    field, prim = base.split(".")
    p = MODS[field]
    edge, rnd = int_rows(base)
    if field in ("fr", "fq"):
        for r in edge + rnd:
            for x, bound in zip(r, TABLE32[prim][0]):
                assert 0 <= x < (R256 if bound is None else bound * p), (name, hex(x))
        return
    for r in edge + rnd:
        if prim == "unpack":
            assert all(0 <= w <= M32 for w in r[0])
        elif prim == "pack":
            assert all(l <= M29 for l in r[0][:8]) and value29(r[0]) < R256
        elif prim == "normalize":
            assert all(l < (1 << 32) - 8 for l in r[0])
        elif prim in ("mul", "mul_cold", "sqr", "sqr_cold", "mul2add"):
            ops = r if len(r) > 1 else (r[0], r[0])
            units = [max(-(-(l + 1) // (1 << 29)) for l in o[:8]) for o in ops]           # limbs < units * 2^29
            assert all(u <= 3 and o[8] < (1 << 27) and value29(o) < 32 * p for u, o in zip(units, ops)), (name, r)
            col = sum(units[2 * k] * units[2 * k + 1] for k in range(len(ops) // 2))
            assert col <= 6, (name, units)                                                # A B (+ C D) < 6.1 in units of 2^58
        elif prim.startswith(("sub", "neg")):
            KI = int(prim[3:])
            b = r[-1]
            assert all(l <= M29 for l in b[:8]) and value29(b) < ((2 << KI) - 1) * p
            assert all(0 <= w <= M32 for w in expected_words(base, r))
        elif prim.startswith("cond_sub") or prim == "canonical":
            assert all(l <= M29 for l in r[0]) and value29(r[0]) < R261
        elif prim == "is_zero_mod_p":
            assert all(l <= M29 for l in r[0][:8]) and value29(r[0]) < 32 * p
        else:
            raise AssertionError("no domain written down for " + name)


def describe(name, ops, got, want, i):
    """one mismatching row, for an assertion message"""
    fmt = lambda w: " ".join("%08x" % int(x) for x in w)
    return "%s row %d\n  operands: %s\n  got:      %s\n  expected: %s" % (name, i, " | ".join(fmt(o[i]) for o in ops), fmt(got[i]), fmt(want[i]))
