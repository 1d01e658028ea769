"""Synthetic plans for the RECIP and ISQRT record kinds with their expected cells in closed form, and the plans both validators must
refuse.

`NormBuilder` is tests/witness_synth.py's `Builder` (imported, left as it is) with one method per new kind.  The expectation is worked
out from the planted values alone and by another route than `ezkl_layout.recip_claim` / `sqrt_claim`, `witness_plan.run_plan_host` or the
kernels take: the reciprocal by SEARCH -- of the integers around S / x, the smallest y that minimises |y * x - S|, which is what the gates
of `optimum_convex_function` accept --, the root by comparing 4 T with (2 r + 1)^2, r = isqrt(T).  A lane the kind must refuse (a value
beyond 62 bits, T >= 2^62) is expected to write nothing: its cell stays zero and it is listed in `refused`.  `CASES` maps a test id to
`make(seed) -> Case`; tests/test_witness_plan_norm_cpu.py holds the host interpreter to the closed form, tests/test_gpu_witness_norm.py the
device columns.  `bad_plans()` lists (the words of the refusal, the record, a plan with that one defect)."""
import math
import random

import witness_synth as S
from ezkl_amd import witness_plan as WP

R, NONE, FIT = S.R, S.NONE, S.FIT
COUNTS = [1, 63, 64, 65, 255, 256, 257]                                  # wave and workgroup edges of the 256-lane kernel
RECIP_SCALES = [1, 1 << 21, FIT - 1]
SQRT_SCALES = [1, 128, (1 << 31) - 1]
ROOTS = [1, (1 << 16) - 1, (1 << 31) - 1]
ZERO_INVERSE = 8192


def recip_expected(x, scale):
    """the smallest integer y that minimises |y * x - S| over the integers, x != 0: found among the integers around S / x"""
    q = scale // x
    f = lambda y: abs(y * x - scale)
    best = min(f(y) for y in range(q - 3, q + 4))
    y = min(y for y in range(q - 3, q + 4) if f(y) == best)
    assert f(y) <= f(y + 1) and f(y) < f(y - 1), "the two inequalities of the gates"
    return y


def sqrt_expected(t):
    """the integer nearest to sqrt(t), t > 0 (no tie: 4 t is no odd square)"""
    r = math.isqrt(t)
    assert 4 * t != (2 * r + 1) ** 2
    return r + 1 if 4 * t > (2 * r + 1) ** 2 else r


class NormBuilder(S.Builder):
    def recip(self, dst, a, scale, zero_inverse=ZERO_INVERSE):
        """a RECIP record over the cells `a` at S = scale; the constant a zero input takes joins the constants section"""
        if zero_inverse % R not in self.consts:
            self.consts.append(zero_inverse % R)
        vals = []
        for v in self._read(a):
            x = S.signed(v)
            vals.append(None if abs(x) >= FIT else zero_inverse if x == 0 else recip_expected(x, scale))
        dst = list(dst)
        ri = len(self.records)
        self.records.append([WP.RECIP, len(dst), scale & NONE, scale >> 32, self._push(dst), self._push(a.idx), self.consts.index(zero_inverse % R), 0])
        return self._write(ri, dst, vals)

    def isqrt(self, dst, a, scale):
        vals = []
        for v in self._read(a):
            x = S.signed(v)
            t = x * scale
            vals.append(None if abs(x) >= FIT or t >= FIT else 0 if t <= 0 else sqrt_expected(t))
        return self._elem(WP.ISQRT, dst, a.idx, vals, p0=scale)


def recip_values(scale):
    """the values the issue names at S = scale, those a lane can hold: 0, +-1, +-2, +-S, +-2S (the ties), 2S +- 1, +-(2S + 1), +-(2^62 - 1)"""
    named = [0, 1, -1, 2, -2, scale, -scale, 2 * scale, -2 * scale, 2 * scale - 1, 2 * scale + 1, -(2 * scale + 1), FIT - 1, -(FIT - 1)]
    return [v for v in named if abs(v) < FIT]


def sqrt_values(scale):
    """inputs x whose T = x * scale is (for scale 1) or brackets (else) each of 0, 1, 2, 3, r^2, r^2 + r, r^2 + r + 1 for r in ROOTS, the
    largest T below 2^62, and negative values"""
    targets = [0, 1, 2, 3] + [t for r in ROOTS for t in (r * r, r * r + r, r * r + r + 1)] + [FIT - 1]
    xs = []
    for t in targets:
        for x in (t // scale, -(-t // scale)):
            if x * scale < FIT and x not in xs:
                xs.append(x)
    return xs + [-1, -(FIT - 1), -((FIT - 1) // scale)]


def too_large(scale):
    """the smallest input whose T = x * scale reaches 2^62 (for scale 1: 2^62 itself, beyond what a lane holds)"""
    return -(-FIT // scale)


def _fill(named, count, rng, draw):
    """`count` values: the named ones first (cycled from a seeded start when they are more), seeded ones after them"""
    at = rng.randrange(len(named))
    vals = [named[(at + i) % len(named)] for i in range(min(count, len(named)))]
    return vals + [draw() for _ in range(count - len(vals))]


def _geometry(count):
    return max(4, (count - 1).bit_length())


def elem_case(kind, count, scale, seed, bad=()):
    """one INPUT record (column 0, seeded rows) and one RECIP / ISQRT record over it (column 1, other seeded rows); bad: {element: value}"""
    rng, where = random.Random(1000 * seed + count + kind), random.Random(count + kind)      # the rows do not follow the seed: one plan per case
    if kind == WP.RECIP:
        bound = min(4 * scale + 2, FIT)
        vals = _fill(recip_values(scale), count, rng, lambda: rng.choice([-1, 1]) * rng.randrange(1, bound))
        if count >= len(recip_values(scale)):
            rng.shuffle(vals)
    else:
        vals = _fill(sqrt_values(scale), count, rng, lambda: rng.randrange(FIT // scale))
        if count >= len(sqrt_values(scale)):
            rng.shuffle(vals)
    for e, v in dict(bad).items():
        vals[e] = v
    k = _geometry(count)
    b = NormBuilder(k, 2)
    src = b.input(b.rows(0, where.sample(range(1 << k), count)), vals)
    rows = b.rows(1, where.sample(range(1 << k), count))
    out = b.recip(rows, src, scale) if kind == WP.RECIP else b.isqrt(rows, src, scale)
    case = S.Case(b, [out.idx[0], out.idx[-1]])                          # (elements 0 and count - 1 are never the refused ones)
    case.unwritten = list(case.refused_cells)
    return case


BAD_AT = (63, 64)                                                        # the refused elements of the 130-element record: the last lane of a wave and the next one's first
BAD_COUNT = 130


def failing_case(kind, scale, bad, seed=0):
    """130 elements; with `bad`, element 63 is 2^62 and element 64 is -2^62 (RECIP) or the smallest input whose T reaches 2^62 (ISQRT; for
    scale 1 that is 2^62 too).  The plan is the same either way and for every seed: only the inputs follow them."""
    worst = {BAD_AT[0]: FIT, BAD_AT[1]: -FIT if kind == WP.RECIP else too_large(scale)}
    return elem_case(kind, BAD_COUNT, scale, seed, worst if bad else {})


def _case(kind, count, scale): return lambda seed: elem_case(kind, count, scale, seed)


CASES = {}
for _count in COUNTS:
    for _scale in RECIP_SCALES:
        CASES["recip-n%d-S%d" % (_count, _scale)] = _case(WP.RECIP, _count, _scale)
    for _scale in SQRT_SCALES:
        CASES["sqrt-n%d-scale%d" % (_count, _scale)] = _case(WP.ISQRT, _count, _scale)


# ---- what the validators refuse ---------------------------------------------------------------------------------------------------------------
def small_plan():
    """0 INPUT (six values), 1 RECIP over the first four at S = 6, 2 ISQRT over the last four at scale 3"""
    b = NormBuilder(4, 3)
    src = b.input(b.rows(0, range(6)), [0, 4, -4, 12, 5, -7])
    rec = b.recip(b.rows(1, range(4)), src.take(range(4)), 6, 99)
    root = b.isqrt(b.rows(2, range(4)), src.take(range(2, 6)), 3)
    return S.Case(b, [rec.idx[0], rec.idx[3], root.idx[1], root.idx[2]])


def _tampered(plan):
    q = WP.WitnessPlan.from_bytes(plan.to_bytes())
    q.records, q.pool = q.records.copy(), q.pool.copy()
    return q


def bad_plans():
    """(the words both validators must use, the record they must name, a plan with that one defect)"""
    plan = small_plan().plan
    P0, P1, DST, A, B_ = 2, 3, 4, 5, 6
    cells = plan.n_advice << plan.k
    out = []

    def bad(words, rec, field=None, value=None, pool_at=None, pool_value=None):
        q = _tampered(plan)
        if field is not None:
            q.records[rec, field] = value & NONE
        if pool_at is not None:
            q.pool[pool_at] = pool_value
        out.append((words, rec, q))

    rec = plan.records.tolist()
    bad("reciprocal scale outside [1, 2^62)", 1, P0, 0)                 # S = 0
    bad("reciprocal scale outside [1, 2^62)", 1, P1, 1 << 30)           # S = 2^62 + 6
    bad("reciprocal scale outside [1, 2^62)", 1, P1, NONE)
    bad("zero-inverse index past the constants", 1, B_, len(plan.consts))
    bad("zero-inverse index past the constants", 1, B_, NONE)
    bad("zero square-root scale", 2, P0, 0)
    bad("a square-root record with a second parameter", 2, P1, 1)
    bad("a square-root record with a second parameter", 2, P1, NONE)
    unwritten = (2 << plan.k) + 15
    bad("a cell is read before an earlier record has written it", 1, pool_at=rec[1][A] + 3, pool_value=unwritten)
    bad("a cell is read before an earlier record has written it", 2, pool_at=rec[2][A], pool_value=plan.pool[rec[2][DST]])       # ... its own destination
    bad("a cell is read before an earlier record has written it", 1, pool_at=rec[1][A], pool_value=plan.pool[rec[2][DST] + 1])  # ... a later record's
    bad("cell index out of range", 1, pool_at=rec[1][A], pool_value=cells)
    bad("cell index out of range", 2, pool_at=rec[2][DST] + 3, pool_value=cells)
    bad("a cell is written twice", 1, pool_at=rec[1][DST] + 1, pool_value=plan.pool[rec[1][DST]])
    bad("a cell is written twice", 2, pool_at=rec[2][DST], pool_value=plan.pool[rec[1][DST]])
    return out
