"""Synthetic plans for the record kinds of the surrogate's ops -- the running sum and product (SUMACC, PRODACC), GATHER and CLAMP -- with their
expected cells in closed form, and the plans both validators must refuse.

`OpsBuilder` is tests/witness_synth.py's `Builder` (imported, left as it is) with one method per new kind: each takes the cells it reads
together with the values planted in them and works out what the record must write with Python integers from those values alone -- a
prefix fold, a list index, min / max.  `CASES` maps a test id to `make(seed) -> Case`; tests/test_witness_plan_ops_cpu.py holds the host
interpreter to the closed form, tests/test_gpu_witness_ops.py the device columns.  `bad_plans()` lists (the words of the refusal, a plan
with that one defect)."""
import random

import witness_synth as S
from ezkl_amd import witness_plan as WP

R, NONE, HALF, FIT = S.R, S.NONE, S.HALF, S.FIT


class OpsBuilder(S.Builder):
    def acc(self, kind, w, scans, phase=0):
        """scans: per scan its steps, (destination cell, w entries: None or (cell, value)).  Step s must hold the fold -- the sum from 0, the
        product from 1 -- of the planted operands of steps 0 .. s; a shorter scan has no steps past its end."""
        nd, ns = len(scans), max(len(sc) for sc in scans)
        dst, a = [NONE] * (ns * nd), [NONE] * (ns * w * nd)
        ri = len(self.records)
        cells, vals = [], []
        for d, steps in enumerate(scans):
            run = 0 if kind == WP.SUMACC else 1
            for s, (cell, row) in enumerate(steps):
                assert len(row) == w
                dst[s * nd + d] = cell
                for j, p in enumerate(row):
                    if p is not None:
                        a[(s * w + j) * nd + d] = p[0]
                        run = (run + p[1]) % R if kind == WP.SUMACC else run * p[1] % R
                cells.append(cell)
                vals.append(run)
        self.records.append([kind, nd, w, ns, self._push(dst), self._push(a), 0, phase])
        return self._write(ri, cells, vals)

    def gather(self, dst, index, table):
        """lane i must hold table.val[s] with s the signed value planted in index cell i; s outside [0, len(table)): refused"""
        n = len(table)
        tv = self._read(table)
        vals = [tv[S.signed(v)] if 0 <= S.signed(v) < n else None for v in self._read(index)]
        return self._elem(WP.GATHER, dst, index.idx, vals, p0=self._push(table.idx), p1=n)

    def clamp(self, dst, a, lo, hi):
        return self._elem(WP.CLAMP, dst, a.idx, [min(max(S.signed(v), lo), hi) % R for v in self._read(a)], p0=lo, p1=hi & NONE)


# ---- the scans -----------------------------------------------------------------------------------------------------------------------------
ACC_KINDS = {"sum": WP.SUMACC, "prod": WP.PRODACC}
# (scans, steps, w): 1 .. 100 steps around the 16-lane chunk edges, 1 .. 9 scans (four to a wave), w = 1 .. 3
ACC_SHAPES = sorted({(5, s, 2) for s in (1, 2, 15, 16, 17, 31, 32, 33, 100)} | {(d, s, w) for d in (1, 3, 4, 5, 9) for s in (17, 33) for w in (1, 2, 3)})


def acc_case(kind, lengths, w, seed, empty=(), partial=False, k=9):
    """scans of the given lengths over full-range operands in column 0 (a product's without the zero), read through seeded indices;
    destinations permuted across columns 1 and 2.  empty: the steps (of every scan that has them) without any operand; partial: rows with
    only some of the w operands"""
    ops = S.field_operands(seed)
    if kind == WP.PRODACC:
        ops = [v for v in ops if v]
    b = OpsBuilder(k, 3)
    n = 1 << k
    src = b.const(b.rows(0, range(len(ops))), ops)
    rng = random.Random(seed + 200)
    total = sum(lengths)
    assert total <= 2 * n
    ends = [n, 3 * n - 1][::1 if seed % 2 else -1]                     # row 0 of column 1, the last row of column 2
    dst = ends[:1] + rng.sample(range(n + 1, 3 * n - 1), max(total - 2, 0)) + ends[1:total]
    pairs = src.pairs()
    scans, at = [], 0
    for d, length in enumerate(lengths):
        steps = []
        for s in range(length):
            row = [None if s in empty or (partial and (s + j + d) % 3 == 0) else pairs[rng.randrange(len(pairs))] for j in range(w)]
            steps.append((dst[at], row))
            at += 1
        scans.append(steps)
    out = b.acc(kind, w, scans)
    return S.Case(b, [steps[-1][0] for steps in scans] + out.idx[:1])


SPECIAL = [1, R - 1, HALF - 1, HALF, HALF + 1, R - 1, R - 1, 2, HALF + 1, (1 << 255) % R, R - 2, 1 << 224]


def special_values_case(kind, seed):
    """the ends of the field in one scan each way: products over 1, r - 1, (r - 1) / 2 +- 1 and the wrapping pair (r - 1)(r - 1), then a zero
    after which every row is zero; sums that wrap past r at every step (r - 1 + r - 1, (r - 1) / 2 + 1 twice).  A second scan runs the
    same values backwards (zero first: a product that is zero from its first row on)."""
    vals = SPECIAL[seed % 3:] + SPECIAL[:seed % 3] + [0, 5, R - 1, 7]
    b = OpsBuilder(7, 3)
    src = b.const(b.rows(0, range(len(vals))), vals)
    pairs = src.pairs()
    fwd = [(b.cell(1, s), [pairs[s]]) for s in range(len(vals))]
    back = [(b.cell(2, 127 - s), [pairs[len(vals) - 1 - s]]) for s in range(len(vals))]
    out = b.acc(kind, 1, [fwd, back])
    if kind == WP.PRODACC:
        assert out.val[len(vals) - 5] != 0 and out.val[len(vals) - 4] == 0 and out.val[len(vals) - 1] == 0 and out.val[len(vals)] == 7
    else:
        assert any(x + y >= R for x, y in zip(out.val, vals[1:]))
    return S.Case(b, [fwd[-1][0], back[-1][0]])


# ---- gather ---------------------------------------------------------------------------------------------------------------------------------
GATHER_LANES = [1, 63, 64, 65, 257]
GATHER_TABLES = [1, 2, 300]


def gather_bad_indices(n):
    """-1, n, +-2^62 and one value per high limb, both signs"""
    return [v % R for v in [-1, n, FIT, -FIT] + [s * (1 << (32 * i)) for i in range(2, 8) for s in (1, -1)]]


def gather_case(lanes, n, pattern, seed, bad=False, k=10):
    """a table of n cells in column 0 (full-range values), `lanes` index cells in column 1, the picks in column 2.  Indices 0 and n - 1 are
    among them; reversed: n - 1, n - 2, ...; fanin: many lanes on the first three rows.  bad: the indices of `gather_bad_indices` at
    seeded lanes, among passing ones."""
    rng = random.Random(seed + 300)
    ops = S.field_operands(seed)
    b = OpsBuilder(k, 3)
    table = b.const(b.fresh(n, corner=True), [ops[(i + 3 * seed) % len(ops)] if i < 2 * len(ops) else rng.randrange(R) for i in range(n)])
    if pattern == "reversed":
        idx = [(n - 1 - i) % n for i in range(lanes)]
    elif pattern == "fanin":
        idx = [(i * 7 + seed) % 3 % n for i in range(lanes)]
    else:
        idx = [rng.randrange(n) for _ in range(lanes)]
    if pattern == "reversed":
        idx[-1] = 0
    else:
        idx[0], idx[-1] = 0, n - 1
    if lanes == 1:
        idx = [(0, n - 1)[seed % 2]]
    assert (0 in idx and n - 1 in idx) or lanes == 1
    idx = [v % R for v in idx]
    if bad:
        wrong = gather_bad_indices(n)
        for at, v in zip(sorted(rng.sample(range(1, lanes - 1), len(wrong))), wrong):
            idx[at] = v
    index = b.const(b.rows(1, rng.sample(range(1 << k), lanes)), idx)
    dst = b.rows(2, range(lanes))
    out = b.gather([dst[p] for p in S.order("permuted", lanes, seed)], index, table)
    assert len(b.refused) == (len(gather_bad_indices(n)) if bad else 0)
    return S.Case(b, [] if bad else [out.idx[0], out.idx[-1]])


def gather_accounting_case(bad, seed=0):
    """two gather records over one column of 600 indices: tables of 4 and of 300 cells.  With `bad`, lanes 5 and 500 hold 4 (past the
    small table only), lanes 64 and 255 hold -1 and 300 (past both).  The plan is the same for every seed: only the inputs follow it."""
    rng = random.Random(seed)
    vals = [rng.randrange(4) for _ in range(600)]
    if bad:
        for at, v in zip((5, 64, 255, 500), (4, -1, 300, 4)):
            vals[at] = v
    b = OpsBuilder(10, 4)
    table = b.const(b.rows(0, range(300)), [random.Random(99 + i).randrange(R) for i in range(300)])
    index = b.input(b.rows(1, range(600)), vals)
    big = b.gather(b.rows(2, range(600)), index, table)
    small = b.gather(b.rows(3, range(1023, 423, -1)), index, table.take(range(4)))
    return S.Case(b, [big.idx[0], small.idx[0]])


# ---- clamp ----------------------------------------------------------------------------------------------------------------------------------
CLAMP_BOUNDS = [(-5, 7), (0, 0), (-(1 << 31), (1 << 31) - 1), (3, 3), (-10, -2), (2, 9), (-(1 << 31), -(1 << 31)), ((1 << 31) - 1, (1 << 31) - 1)]


def clamp_case(seed):
    """per bounds: lo - 1, lo, 0, hi, hi + 1, r - 1, both sides of the sign change and of 2^62, and a value per high limb of either sign"""
    b = OpsBuilder(9, 2)
    outs = []
    for i, (lo, hi) in enumerate(CLAMP_BOUNDS):
        vals = [lo - 1, lo, 0, hi, hi + 1, -1, HALF - 1, HALF, HALF + 1, FIT - 1, -(FIT - 1), FIT, -FIT] + [s * (1 << (32 * j)) for j in range(2, 8) for s in (1, -1)]
        vals = [v % R for v in vals[(i + seed) % 5:] + vals[:(i + seed) % 5]]
        src = b.const(b.fresh(len(vals), corner=i % 3 == 0), vals)
        outs.append(b.clamp(b.fresh(len(vals), corner=i % 3 == 1), src, lo, hi))
    return S.Case(b, [o.idx[0] for o in outs])


def _acc(kind, lengths, w, **kw): return lambda seed: acc_case(kind, lengths, w, seed, **kw)
def _special(kind): return lambda seed: special_values_case(kind, seed)
def _gather(lanes, n, pattern, bad=False): return lambda seed: gather_case(lanes, n, pattern, seed, bad)


CASES = {}
for _name, _kind in ACC_KINDS.items():
    for _nd, _ns, _w in ACC_SHAPES:
        CASES["%s-scans%d-steps%d-w%d" % (_name, _nd, _ns, _w)] = _acc(_kind, [_ns] * _nd, _w)
    CASES["%s-ragged-1-5-16-17-33" % _name] = _acc(_kind, [1, 5, 16, 17, 33], 2)
    CASES["%s-ragged-33-17-16-5-1-w3" % _name] = _acc(_kind, [33, 17, 16, 5, 1], 3)
    CASES["%s-operandless-steps17" % _name] = _acc(_kind, [17] * 5, 2, empty=(0, 1, 2))              # chunk = 2: steps 0, chunk - 1, chunk
    CASES["%s-operandless-steps33" % _name] = _acc(_kind, [33] * 5, 2, empty=(0, 2, 3))              # chunk = 3
    CASES["%s-operandless-steps100" % _name] = _acc(_kind, [100] * 3, 1, empty=(0, 6, 7, 13, 14, 99))  # chunk = 7
    CASES["%s-partial-operandless-ragged" % _name] = _acc(_kind, [1, 5, 16, 17, 33, 32], 3, empty=(0, 2, 3), partial=True)
    CASES["%s-special-values" % _name] = _special(_kind)
for _lanes in GATHER_LANES:
    for _n in GATHER_TABLES:
        CASES["gather-lanes%d-table%d" % (_lanes, _n)] = _gather(_lanes, _n, "random")
for _n in GATHER_TABLES:
    CASES["gather-reversed-table%d" % _n] = _gather(257, _n, "reversed")
    CASES["gather-fanin-table%d" % _n] = _gather(257, _n, "fanin")
    CASES["gather-outside-table%d-lanes65" % _n] = _gather(65, _n, "random", bad=True)
    CASES["gather-outside-table%d-lanes257" % _n] = _gather(257, _n, "fanin", bad=True)
CASES["clamp-bounds-and-edges"] = clamp_case


# ---- what the validators refuse ---------------------------------------------------------------------------------------------------------------
def small_plan():
    """one record of each new kind over nine constants: 0 CONST, 1 SUMACC, 2 PRODACC, 3 GATHER, 4 CLAMP"""
    b = OpsBuilder(4, 3)
    src = b.const(b.rows(0, range(9)), [5, 6, 7, 8, 9, 10, 0, 1, 2])
    p = src.pairs()
    b.acc(WP.SUMACC, 1, [[(b.cell(1, 3 * d + s), [p[3 * d + s]]) for s in range(3)] for d in range(2)])
    b.acc(WP.PRODACC, 1, [[(b.cell(1, 8 + 3 * d + s), [p[3 * d + s]]) for s in range(3)] for d in range(2)])
    b.gather(b.rows(2, range(3)), src.take(range(6, 9)), src.take(range(3)))
    b.clamp(b.rows(2, range(4, 7)), src.take(range(3)), -1, 6)
    return S.Case(b, [b.cell(2, 0)])


def _tampered(plan):
    q = WP.WitnessPlan.from_bytes(plan.to_bytes())
    q.records, q.pool = q.records.copy(), q.pool.copy()
    return q


def bad_plans():
    """(the words both validators must use, the record they must name, a plan with that one defect)"""
    plan = small_plan().plan
    KIND, COUNT, P0, P1, DST, A = range(6)
    n_words, cells = len(plan.pool), plan.n_advice << plan.k
    out = []

    def bad(words, rec, field=None, value=None, pool_at=None, pool_value=None):
        q = _tampered(plan)
        if field is not None:
            q.records[rec, field] = value & NONE
        if pool_at is not None:
            q.pool[pool_at] = pool_value
        out.append((words, rec, q))

    rec = plan.records.tolist()
    for r in (1, 2):
        bad("bad scan shape", r, P0, 0)
        bad("bad scan shape", r, P1, 0)
        bad("bad scan shape", r, DST, n_words - 5)                  # six destination words from there: one past the pool
        bad("bad scan shape", r, A, n_words + 1)
        bad("bad scan shape", r, P1, n_words)                       # more steps than the pool has words
    bad("empty gather table", 3, P1, 0)
    bad("gather table runs past the pool", 3, P1, n_words - rec[3][P0] + 1)
    bad("gather table runs past the pool", 3, P0, n_words + 1)
    bad("gather table runs past the pool", 3, P1, NONE)
    bad("bad clamp bounds", 4, P0, 7)                               # lo = 7 > hi = 6
    bad("bad clamp bounds", 4, P1, -2)                              # hi = -2 < lo = -1
    unwritten = (2 << plan.k) + 15
    bad("a cell is read before an earlier record has written it", 3, pool_at=rec[3][P0] + 1, pool_value=unwritten)       # a listed cell no record writes
    bad("a cell is read before an earlier record has written it", 3, pool_at=rec[3][P0] + 2, pool_value=plan.pool[rec[3][DST]])   # ... or the record itself does
    bad("cell index out of range", 3, pool_at=rec[3][P0], pool_value=cells)
    bad("a cell is read before an earlier record has written it", 3, pool_at=rec[3][A], pool_value=unwritten)
    bad("a cell is read before an earlier record has written it", 1, pool_at=rec[1][A] + 2, pool_value=unwritten)
    bad("a cell is read before an earlier record has written it", 4, pool_at=rec[4][A], pool_value=unwritten)
    bad("cell index out of range", 2, pool_at=rec[2][A], pool_value=cells)
    bad("a cell is written twice", 1, pool_at=rec[1][DST] + 1, pool_value=plan.pool[rec[1][DST]])
    bad("a cell is written twice", 2, pool_at=rec[2][DST], pool_value=plan.pool[rec[1][DST]])
    return out
