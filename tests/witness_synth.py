"""Synthetic witness plans for the kernels of csrc/witness.hip, with their expected cells in closed form.

Plans recorded from circuits hold small integers in few shapes.  `Builder` assembles a `WitnessPlan` record by record -- index arrays
appended to the pool, the record's eight words, the cell count -- from PLANTED values: arbitrary field elements enter through CONST
records (32 canonical bytes each), 64-bit integers through INPUT and PARAM.  Every method that adds a record takes the cells it reads
together with the values planted in them (`Cells`) and works out what the record must write with Python integers from those values
alone: (a + b) % R, pow(a, R - 2, R), the digits of |s|, prefix sums of the planted products.  Nothing here decodes a pool or walks a
record list, so the expectation shares no code and no reading of the format with `witness_plan.run_plan_host` or with the kernels.  A
lane the kind must refuse (a value beyond its range) is expected to write nothing: its cell stays zero and it is listed in `refused`.

`CASES` maps a test id to `make(seed) -> Case`; the CPU file compares the host interpreter with the closed form, the GPU file the
device columns.  Everything is seeded: the same id and seed give the same bytes."""
import random

from ezkl_amd import witness_plan as WP

R, NONE = WP.R, WP.NONE
HALF = (R - 1) // 2
INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)
FIT = 1 << 62                                      # what a lane holds of a signed value: |s| < 2^62


def signed(v):
    """the signed integer a canonical field element stands for: from (r - 1) / 2 on it is negative"""
    return v - R if 2 * v >= R - 1 else v


def field_operands(seed):
    """the ends of the field, the three elements around the sign change, one element per limb (and 2^32 * i), 2^255 mod r, 32 seeded
    uniform ones"""
    rng = random.Random(seed)
    return ([0, 1, R - 1, HALF - 1, HALF, HALF + 1] + [1 << (32 * i) for i in range(1, 8)] + [(1 << 32) * i for i in range(1, 8)] + [(1 << 255) % R] +
            [rng.randrange(R) for _ in range(32)])


# a + b >= r (to 2r - 2, to exactly r, to r + 1), a - b < 0, (r - 1)^2
WRAP_PAIRS = [(R - 1, R - 1), (R - 1, 1), (HALF + 1, HALF), (0, 1), (0, R - 1), (HALF, HALF + 1), (1, R - 1), (HALF + 1, HALF + 1), (R - 2, 2)]
INT_OPERANDS = [0, 1, -1, INT64_MAX, INT64_MIN, 1 << 62, -(1 << 62), (1 << 63) - 1, -((1 << 63) - 1)]
PATTERNS = ["contiguous", "reversed", "permuted", "fanin"]


def order(pattern, count, seed):
    """the positions 0 .. count - 1 in order, backwards, as a seeded permutation, or -- many lanes on one entry -- folded onto the first three"""
    base = list(range(count))
    if pattern == "contiguous":
        return base
    if pattern == "reversed":
        return base[::-1]
    random.Random(seed).shuffle(base)
    return [p % 3 for p in base] if pattern == "fanin" else base


class Cells:
    """advice cells and the values planted in them (None: a cell its record must leave unwritten)"""

    def __init__(self, idx, val):
        self.idx, self.val = list(idx), list(val)
        assert len(self.idx) == len(self.val)

    def take(self, positions):
        return Cells([self.idx[i] for i in positions], [self.val[i] for i in positions])

    def pairs(self):
        return list(zip(self.idx, self.val))

    def __len__(self):
        return len(self.idx)


def _digits(mag, base, legs):
    out = []
    for _ in range(legs):
        mag, d = divmod(mag, base)
        out.append(d)
    assert mag == 0
    return out


class Builder:
    def __init__(self, k, n_advice, n_phases=1, n_challenges=0):
        self.k, self.n, self.n_advice, self.n_phases, self.n_challenges = k, 1 << k, n_advice, n_phases, n_challenges
        self.pool, self.records, self.consts, self.params, self.x = [], [], [], [], []
        self.tables, self.table_values = [], []
        self.n_cells = 0
        self.expect = {}                           # cell -> the canonical value it must hold after the run (a refused cell: 0)
        self.refused = []                          # (record, element, cell) of every lane that must report itself and leave its cell alone
        self.dot_totals = []                       # (last live cell, sum of a * b mod r over the whole dot)
        self._corners = []
        for c in (self.cell(0, 0), self.cell(0, self.n - 1), self.cell(n_advice - 1, 0), self.cell(n_advice - 1, self.n - 1)):
            if c not in self._corners:
                self._corners.append(c)
        self._reserved, self._next = set(self._corners), 0

    def cell(self, col, row):
        assert 0 <= col < self.n_advice and 0 <= row < self.n
        return (col << self.k) + row

    def rows(self, col, rows):
        return [self.cell(col, r) for r in rows]

    def fresh(self, count, corner=False):
        """`count` unused cells along the linear coordinate (across column ends); with `corner`, one of them is row 0 or row 2^k - 1 of the
        first or the last column, as long as one of the four is left"""
        out = [self._corners.pop(0)] if corner and self._corners else []
        while len(out) < count:
            c, self._next = self._next, self._next + 1
            if c not in self._reserved:
                out.append(c)
        assert self._next <= self.n_advice << self.k
        return out

    # ---- the blob's parts ----------------------------------------------------------------------------------------------------------------
    def _push(self, words):
        off = len(self.pool)
        self.pool += [int(w) for w in words]
        return off

    def _write(self, ri, dst, vals):
        for i, (c, v) in enumerate(zip(dst, vals)):
            assert c not in self.expect, "cell %d is planted twice" % c
            if v is None:
                self.refused.append((ri, i, c))
            self.expect[c] = 0 if v is None else v % R
        self.n_cells += len(dst)
        return Cells(dst, [None if v is None else v % R for v in vals])

    def _elem(self, kind, dst, a, vals, b=None, p0=0, p1=0, phase=0):
        dst, a = list(dst), list(a)
        assert len(dst) == len(a) == len(vals) and (b is None or len(b) == len(dst)) and dst
        ri = len(self.records)
        self.records.append([kind, len(dst), p0 & NONE, p1, self._push(dst), self._push(a), self._push(b) if b is not None else 0, phase])
        return self._write(ri, dst, vals)

    @staticmethod
    def _read(src):
        assert None not in src.val, "nothing reads a refused cell"
        return src.val

    def table(self, lo, col_size, values):
        self.tables.append((lo, len(values), col_size, len(self.table_values)))
        self.table_values += [int(v) for v in values]
        return len(self.tables) - 1

    def plan(self, outputs=()):
        return WP.WitnessPlan(self.k, self.n_advice, len(self.x), self.params, self.consts, self.records, list(outputs), self.pool, self.n_cells, len(self.records),
                              b"\0" * 32, self.tables, self.table_values, self.n_challenges, self.n_phases)

    # ---- planted values --------------------------------------------------------------------------------------------------------------------
    def const(self, dst, values, phase=0):
        assert all(0 <= v < R for v in values)
        at = len(self.consts)
        self.consts += list(values)
        return self._elem(WP.CONST, dst, range(at, at + len(values)), values, phase=phase)

    def _ints(self, kind, table, dst, values, positions):
        assert all(INT64_MIN <= v <= INT64_MAX for v in values)
        at = len(table)
        table += list(values)
        positions = range(len(values)) if positions is None else positions
        return self._elem(kind, dst, [at + p for p in positions], [values[p] % R for p in positions])

    def input(self, dst, values, positions=None):
        """lane i reads the positions[i]-th of `values`, which join the plan's input vector"""
        return self._ints(WP.INPUT, self.x, dst, values, positions)

    def param(self, dst, values, positions=None):
        return self._ints(WP.PARAM, self.params, dst, values, positions)

    # ---- the element-wise kinds: what the record must write, from the planted values --------------------------------------------------------
    def copy(self, dst, src, phase=0):
        return self._elem(WP.COPY, dst, src.idx, self._read(src), phase=phase)

    def add(self, dst, a, b):
        return self._elem(WP.ADD, dst, a.idx, [(x + y) % R for x, y in zip(self._read(a), self._read(b))], b.idx)

    def sub(self, dst, a, b):
        return self._elem(WP.SUB, dst, a.idx, [(x - y) % R for x, y in zip(self._read(a), self._read(b))], b.idx)

    def mul(self, dst, a, b):
        return self._elem(WP.MUL, dst, a.idx, [x * y % R for x, y in zip(self._read(a), self._read(b))], b.idx)

    def invz(self, dst, a):
        vals = [pow(x, R - 2, R) for x in self._read(a)]
        assert all(x * inv % R == (x != 0) for x, inv in zip(a.val, vals))
        return self._elem(WP.INVZ, dst, a.idx, vals)

    def hint(self, dst, a, base, legs, es, phase=0):
        """es[i] = NONE: the sign of the signed value, else its digit es[i] in `base`; |s| >= base^legs: refused"""
        vals = []
        for v, e in zip(self._read(a), es):
            s = signed(v)
            if abs(s) >= base ** legs:
                vals.append(None)
            elif e == NONE:
                vals.append(0 if s == 0 else 1 if s > 0 else R - 1)
                assert vals[-1] in (0, 1, R - 1)
            else:
                digits = _digits(abs(s), base, legs)
                assert sum(d * base ** i for i, d in enumerate(digits)) == abs(s) and all(0 <= d < base for d in digits)
                vals.append(digits[e])
        return self._elem(WP.HINT, dst, a.idx, vals, list(es), p0=base, p1=legs, phase=phase)

    def rcidx(self, dst, a, lo, col_size):
        vals = [None if abs(signed(v)) >= FIT else abs(signed(v) - lo) // col_size for v in self._read(a)]
        return self._elem(WP.RCIDX, dst, a.idx, vals, p0=lo, p1=col_size)

    def lookup(self, dst, a, table):
        lo, n, _, off = self.tables[table]
        vals = [self.table_values[off + signed(v) - lo] % R if lo <= signed(v) <= lo + n - 1 else None for v in self._read(a)]
        return self._elem(WP.TABLE, dst, a.idx, vals, p0=table)

    def lookup_index(self, dst, a, table):
        lo, n, col_size, _ = self.tables[table]
        vals = [(signed(v) - lo) // col_size if lo <= signed(v) <= lo + n - 1 else None for v in self._read(a)]
        return self._elem(WP.TBLIDX, dst, a.idx, vals, p0=table)

    def divc(self, dst, a, d):
        """s / d rounded half away from zero, as floor(|s| / d + 1 / 2) with the sign put back; |s| >= 2^52: refused"""
        vals = []
        for v in self._read(a):
            s = signed(v)
            q = (2 * abs(s) + d) // (2 * d)
            vals.append(None if abs(s) >= 1 << 52 else (-q if s < 0 else q) % R)
        return self._elem(WP.DIVC, dst, a.idx, vals, p0=d)

    # ---- the scans -------------------------------------------------------------------------------------------------------------------------
    def dot(self, w, dots, phase=0):
        """dots: per dot its steps, (destination cell, w entries: None or ((cell, value), (cell, value))).  Step s must hold the sum of the
        planted products of steps 0 .. s mod r; a shorter dot has no steps past its end."""
        nd, ns = len(dots), max(len(d) for d in dots)
        dst, a, b = [NONE] * (ns * nd), [NONE] * (ns * w * nd), [NONE] * (ns * w * nd)
        ri = len(self.records)
        cells, vals = [], []
        for d, steps in enumerate(dots):
            products = []
            for s, (cell, row) in enumerate(steps):
                assert len(row) == w
                dst[s * nd + d] = cell
                for j, p in enumerate(row):
                    if p is not None:
                        (ia, va), (ib, vb) = p
                        a[(s * w + j) * nd + d], b[(s * w + j) * nd + d] = ia, ib
                        products.append(va * vb)
                cells.append(cell)
                vals.append(sum(products) % R)
            self.dot_totals.append((steps[-1][0], sum(va * vb for _, row in steps for p in row if p is not None for (_, va), (_, vb) in [p]) % R))
        self.records.append([WP.DOT, nd, w, ns, self._push(dst), self._push(a), self._push(b), phase])
        return self._write(ri, cells, vals)

    def rlc(self, dst, src, count, challenge, c, phase=1):
        """count scans, step-major: out[t] = sum over u <= t of c^(t - u + 1) * v[u], with the challenge's value c known to the case"""
        steps = len(src) // count
        assert steps * count == len(src) == len(dst)
        v = self._read(src)
        vals = [sum(pow(c, t - u + 1, R) * v[u * count + d] for u in range(t + 1)) % R for t in range(steps) for d in range(count)]
        ri = len(self.records)
        self.records.append([WP.RLC, count, challenge, steps, self._push(dst), self._push(src.idx), 0, phase])
        return self._write(ri, list(dst), vals)


class Case:
    def __init__(self, b, outputs=(), challenges=None):
        self.plan, self.x, self.challenges = b.plan(outputs), list(b.x), challenges
        self.expect, self.dot_totals = dict(b.expect), list(b.dot_totals)
        self.refused, self.refused_cells = sorted(r[:2] for r in b.refused), [r[2] for r in b.refused]

    def columns(self):
        n = 1 << self.plan.k
        return [[self.expect.get(c * n + r, 0) for r in range(n)] for c in range(self.plan.n_advice)]

    def outputs(self):
        return [self.expect[c] for c in self.plan.outputs.tolist()]


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------
ELEM_COUNTS = [1, 63, 64, 65, 255, 256, 257, 513]


def elementwise_case(count, pattern, seed, k=10):
    """CONST a, CONST b, then COPY, ADD, SUB, MUL, INVZ of them and INPUT, PARAM, `count` lanes each, destinations and sources in `pattern`.
    Four of the records own one of the four corner cells (row 0 / row 2^k - 1 of the first / last column)."""
    ops = field_operands(seed)
    A = [ops[(i + 5 * seed) % len(ops)] for i in range(count)]
    B = [ops[(7 * i + i // len(ops) + 3 * seed) % len(ops)] for i in range(count)]
    for i in range(min(count, len(WRAP_PAIRS))):
        A[i], B[i] = WRAP_PAIRS[(i + seed) % len(WRAP_PAIRS)]
    b = Builder(k, -(-(9 * count + 4) >> k) + 1)
    rec = [0]

    def dst():
        rec[0] += 1
        cells = b.fresh(count, corner=(rec[0] + seed) % 2 == 0)
        return [cells[p] for p in order("permuted" if pattern == "fanin" else pattern, count, seed + rec[0])]

    ca, cb = b.const(dst(), A), b.const(dst(), B)
    pa, pb = order(pattern, count, seed + 11), order(pattern, count, seed + 12)
    sa, sb = ca.take(pa), cb.take(pb)
    outs = [b.copy(dst(), sa), b.add(dst(), sa, sb), b.sub(dst(), sa, sb), b.mul(dst(), sa, sb), b.invz(dst(), sa)]
    rng = random.Random(1000 + seed)
    ints = [INT_OPERANDS[(i + seed) % len(INT_OPERANDS)] if i < 2 * len(INT_OPERANDS) else rng.randrange(INT64_MIN, INT64_MAX + 1) for i in range(count)]
    outs.append(b.input(dst(), ints, order(pattern, count, seed + 13)))
    outs.append(b.param(dst(), ints[::-1], order(pattern, count, seed + 14)))
    return Case(b, [o.idx[0] for o in outs] + [outs[3].idx[-1]])


def max_advice_case(seed):
    """n_advice = 64 at k = 4: records on columns 0, 31 and 63"""
    b = Builder(4, 64)
    ops = field_operands(seed)
    c0 = b.const(b.rows(0, range(16)), [ops[(i + 9 * seed) % len(ops)] for i in range(16)])
    c31 = b.copy(b.rows(31, range(15, -1, -1)), c0)
    m = b.mul(b.rows(63, order("permuted", 8, seed)), c0.take(range(8)), c31.take(range(8, 16)))
    steps = lambda d: [(b.cell(63, 8 + 4 * d + s), [(c0.pairs()[4 * d + s], c31.pairs()[s + d])]) for s in range(4)]
    d = b.dot(1, [steps(0), steps(1)])
    return Case(b, [m.idx[0], d.idx[-1], b.cell(63, 8)])


HINT_SHAPES = [(2, 1), (2, 61), (3, 39), (128, 2), ((1 << 31) - 1, 2), ((1 << 32) - 1, 1)]


def hint_case(base, legs, seed, refuse=False):
    """every value under every digit index and the sign; `refuse`: the values at and just past base^legs, among passing ones"""
    bound = base ** legs
    assert bound < FIT
    rng = random.Random(seed)
    vals = [0, 1, -1, base - 1, -(base - 1), bound - 1, -(bound - 1)] + [rng.randrange(-bound + 1, bound) for _ in range(6)]
    if base < bound:
        vals += [base, -base]
    if refuse:
        vals = [1, bound, -bound, 0, bound + 1, -(bound + 1), -(bound - 1), FIT - 1, -(FIT - 1), INT64_MIN, INT64_MAX, bound - 1]
    vals = vals[seed % 3:] + vals[:seed % 3]
    es = [NONE] + (list(range(legs)) if legs == 61 else sorted({0, min(1, legs - 1), legs - 1}))
    b = Builder(10, 2)
    src = b.input(b.fresh(len(vals), corner=True), vals)
    lanes = [(i, e) for i in range(len(vals)) for e in es]
    random.Random(seed + 1).shuffle(lanes)
    dst = b.fresh(len(lanes), corner=True)
    dst = [dst[p] for p in order("permuted", len(lanes), seed + 2)]
    out = b.hint(dst, src.take([i for i, _ in lanes]), base, legs, [e for _, e in lanes])
    return Case(b, [] if refuse else out.idx[:4])


def rcidx_case(seed):
    b = Builder(8, 2)
    recs = [(lo, cs) for lo in (0, -5, 5, -(1 << 31), (1 << 31) - 1) for cs in (1, 3, (1 << 32) - 1)]
    vals = sorted({s for lo, _ in recs for s in (lo, lo + 1, lo - 1, 0, FIT - 1, -(FIT - 1))})
    random.Random(seed).shuffle(vals)
    src = b.input(b.fresh(len(vals), corner=True), vals)
    outs = []
    for i, (lo, cs) in enumerate(recs):
        want = [lo, lo + 1, lo - 1, 0, FIT - 1, -(FIT - 1)]
        want = want[(i + seed) % 6:] + want[:(i + seed) % 6]
        outs.append(b.rcidx(b.fresh(6, corner=i % 4 == 1), src.take([vals.index(s) for s in want]), lo, cs))
    return Case(b, [o.idx[0] for o in outs])


TABLE_LO, TABLE_COL = -8, 5
TABLE_VALUES = [x * x * x - 3 for x in range(TABLE_LO, TABLE_LO + 16)]        # both signs
REFUSE_KINDS = {"decompose": WP.HINT, "range_check": WP.RCIDX, "nonlinearity": WP.TABLE, "nonlinearity_index": WP.TBLIDX, "div": WP.DIVC}


def too_large():
    """what no lane holds in 64 bits as sign and magnitude below 2^62"""
    mags = [FIT, FIT + (1 << 32)] + [1 << (32 * i) for i in range(2, 8)]
    return [v % R for m in mags for v in (m, -m)] + [HALF - 1, HALF, HALF + 1]


def refuse_case(name, seed):
    """one column of constants read by one record of the kind: its own in-range maxima pass, every value of `too_large` is reported and
    not written"""
    kind = REFUSE_KINDS[name]
    good = {WP.HINT: [(1 << 61) - 1, -((1 << 61) - 1), 0], WP.RCIDX: [FIT - 1, -(FIT - 1), 0], WP.TABLE: [TABLE_LO, TABLE_LO + 15, 0],
            WP.TBLIDX: [TABLE_LO, TABLE_LO + 15, 0], WP.DIVC: [(1 << 52) - 1, -((1 << 52) - 1), 0]}[kind]
    vals = [v % R for v in good] + too_large()
    random.Random(seed).shuffle(vals)
    b = Builder(6, 2)
    src = b.const(b.fresh(len(vals), corner=True), vals)
    dst = b.fresh(len(vals), corner=True)
    if kind == WP.HINT:
        b.hint(dst, src, 2, 61, [(NONE, 0, 60)[i % 3] for i in range(len(vals))])
    elif kind == WP.RCIDX:
        b.rcidx(dst, src, -5, 3)
    elif kind == WP.DIVC:
        b.divc(dst, src, 3)
    else:
        t = b.table(TABLE_LO, TABLE_COL, TABLE_VALUES)
        (b.lookup if kind == WP.TABLE else b.lookup_index)(dst, src, t)
    assert len(b.refused) == len(too_large())
    return Case(b)


ACCOUNT_BAD = (3, 64, 255, 256, 700)


def accounting_case(variant, bad=True, seed=0):
    """800 inputs in column 0 read by HINT, RCIDX, HINT.  variant 0: (128, 2) then (2, 61); variant 1: the other way round.  With `bad`,
    elements 3, 64, 255, 256 and 700 hold values that fail a known subset of the three records."""
    rng = random.Random(seed)
    vals = [rng.randrange(-16383, 16384) for _ in range(800)]
    if bad:
        # element: 3 past (128, 2) only | 64 past both decompositions | 255, 256 past everything | 700 past (128, 2) only, negative
        for at, v in zip(ACCOUNT_BAD, (16384, 1 << 61, 1 << 62, INT64_MIN, -16384)):
            vals[at] = v
    b = Builder(10, 4)
    src = b.input(b.rows(0, range(800)), vals)
    shapes = [(128, 2), (2, 61)][::-1 if variant else 1]
    es = lambda legs: [(NONE, 0, legs - 1)[i % 3] for i in range(800)]
    h1 = b.hint(b.rows(1, range(800)), src, shapes[0][0], shapes[0][1], es(shapes[0][1]))
    rc = b.rcidx(b.rows(2, range(223, 1023)), src, -5, 3)
    h2 = b.hint(b.rows(3, range(1023, 223, -1)), src, shapes[1][0], shapes[1][1], es(shapes[1][1]))
    return Case(b, [h1.idx[0], rc.idx[0], h2.idx[799]])


DOT_SHAPES = sorted({(5, s, 2) for s in (1, 2, 15, 16, 17, 31, 32, 33, 100)} | {(d, s, w) for d in (1, 3, 4, 5, 9) for s in (17, 33) for w in (1, 2, 3)})


def dot_case(lengths, w, seed, empty=(), partial=False, k=9):
    """dots of the given lengths over full-range operands in column 0, read through permuted indices; destinations permuted across
    columns 1 and 2.  empty: the steps (of every dot that has them) without any product; partial: rows with only some of the w products"""
    ops = field_operands(seed)
    for i, (x, y) in enumerate(WRAP_PAIRS):                          # (r - 1)^2 and its neighbours among the products
        ops[i], ops[len(ops) - 1 - i] = x, y
    b = Builder(k, 3)
    n = 1 << k
    src = b.const(b.rows(0, range(len(ops))), ops)
    rng = random.Random(seed + 100)
    total = sum(lengths)
    assert total <= 2 * n
    ends = [n, 3 * n - 1][::1 if seed % 2 else -1]                     # row 0 of column 1, the last row of column 2
    dst = ends[:1] + rng.sample(range(n + 1, 3 * n - 1), max(total - 2, 0)) + ends[1:total]
    pairs = src.pairs()
    dots, at = [], 0
    for d, length in enumerate(lengths):
        steps = []
        for s in range(length):
            row = []
            for j in range(w):
                ia = rng.randrange(len(pairs))                       # a wrapping pair with its partner, anything else with a walking index
                ib = len(pairs) - 1 - ia if ia < len(WRAP_PAIRS) else (s * w + j + d) % len(pairs)
                row.append(None if s in empty or (partial and (s + j + d) % 3 == 0) else (pairs[ia], pairs[ib]))
            steps.append((dst[at], row))
            at += 1
        dots.append(steps)
    b.dot(w, dots)
    return Case(b, [cell for cell, _ in b.dot_totals])


PHASED_SCANS, PHASED_STEPS = 3, 40


def large_challenge(seed):
    return random.Random(0xc4a1 + seed).randrange(1 << 250, R)


def three_phase_case(c, seed):
    """phase 0: INPUT -> column 0; phase 1: RLC of column 0 with challenge 0 (= c) -> column 1, HINT (128, 2) of column 1 -> column 2;
    phase 2: COPY of column 2 and a DOT over columns 1 and 2 -> column 3, where the outputs are.  c = 1: the scan holds prefix sums of
    small inputs and everything passes."""
    m = PHASED_SCANS * PHASED_STEPS
    rng = random.Random(seed)
    vals = [rng.randrange(-50, 51) or 1 for _ in range(m)]
    b = Builder(9, 4, n_phases=3, n_challenges=1)
    src = b.input(b.rows(0, random.Random(77).sample(range(512), m)), vals)      # the plan is the same for every seed and challenge
    scan = b.rlc(b.rows(1, range(511, 511 - m, -1)), src, PHASED_SCANS, 0, c)
    lanes = [(i, e) for i in range(m) for e in (NONE, 0, 1)]
    hint = b.hint(b.rows(2, range(len(lanes))), scan.take([i for i, _ in lanes]), 128, 2, [e for _, e in lanes], phase=1)
    if b.refused:                                                     # a failing phase 1: phase 2 never runs, its cells are not expected
        return Case(b, challenges=[c])
    copied = b.copy(b.rows(3, range(len(lanes))), hint, phase=2)
    sp, hp = scan.pairs(), hint.pairs()
    dots = [[(b.cell(3, 400 + 20 * d + s), [(sp[(7 * d + s) % m], hp[(3 * s + j + d) % len(hp)]) for j in range(2)]) for s in range(17 + d)] for d in range(5)]
    b.dot(2, dots, phase=2)
    return Case(b, [cell for cell, _ in b.dot_totals] + copied.idx[:3], challenges=[c])


def _elem(count, pattern): return lambda seed: elementwise_case(count, pattern, seed)
def _hint(base, legs, refuse): return lambda seed: hint_case(base, legs, seed, refuse)
def _refuse(name): return lambda seed: refuse_case(name, seed)
def _dot(lengths, w, **kw): return lambda seed: dot_case(lengths, w, seed, **kw)


CASES = {}
for _count in ELEM_COUNTS:
    for _pattern in PATTERNS:
        CASES["elem-count%d-%s" % (_count, _pattern)] = _elem(_count, _pattern)
CASES["elem-advice64-k4"] = max_advice_case
for _base, _legs in HINT_SHAPES:
    CASES["hint-base%d-legs%d" % (_base, _legs)] = _hint(_base, _legs, False)
    CASES["hint-base%d-legs%d-past-the-range" % (_base, _legs)] = _hint(_base, _legs, True)
CASES["rcidx-lo-colsize-edges"] = rcidx_case
for _name in REFUSE_KINDS:
    CASES["refuse-%s" % _name] = _refuse(_name)
for _nd, _ns, _w in DOT_SHAPES:
    CASES["dot-dots%d-steps%d-w%d" % (_nd, _ns, _w)] = _dot([_ns] * _nd, _w)
CASES["dot-ragged-1-5-16-17-33"] = _dot([1, 5, 16, 17, 33], 2)
CASES["dot-ragged-33-17-16-5-1-w3"] = _dot([33, 17, 16, 5, 1], 3)
CASES["dot-productless-steps17"] = _dot([17] * 5, 2, empty=(0, 1, 2))            # chunk = 2: steps 0, chunk - 1, chunk
CASES["dot-productless-steps33"] = _dot([33] * 5, 2, empty=(0, 2, 3))            # chunk = 3
CASES["dot-productless-steps100"] = _dot([100] * 3, 1, empty=(0, 6, 7, 13, 14, 99))  # chunk = 7
CASES["dot-partial-steps17-w3"] = _dot([17] * 5, 3, partial=True)
CASES["dot-partial-steps33-w2"] = _dot([33] * 4, 2, partial=True)
CASES["dot-partial-productless-ragged"] = _dot([1, 5, 16, 17, 33, 32], 3, empty=(0, 2, 3), partial=True)
