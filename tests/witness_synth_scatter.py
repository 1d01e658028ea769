"""Synthetic plans for the SCATTER, COMPLEMENT and ONEHOT record kinds with their expected cells in closed form, and the plans both
validators must refuse.

`IndexedBuilder` is tests/witness_synth.py's `Builder` (imported, left as it is) with one method per new kind.  The expectations are worked
out from the planted values alone: a scatter is "a copy of the base, then `out[s * mult + off] = src` element by element" on a Python list,
a complement is `sorted(set(range(n)) - set(sources))[:count]`, a one-hot entry is `int(s == position)`; nothing here decodes a pool or walks
a record list, so it shares no code with `witness_plan.run_plan_host` or with the kernels.  A SCATTER with an index outside its dimension is
expected to leave ALL its cells unwritten (they stay zero and are listed in `unwritten`; the offending ELEMENTS are listed in `refused`); a
ONEHOT lane with an index outside the classes leaves its own cell.  `CASES` maps a test id to `make(seed) -> IndexedCase`;
tests/test_witness_plan_scatter_cpu.py holds the host interpreter to the closed form, tests/test_gpu_witness_scatter.py the device columns.
`bad_plans()` lists (the words of the refusal, the record, a plan with that one defect)."""
import random

import witness_synth as S
from ezkl_amd import witness_plan as WP

R, NONE, FIT = S.R, S.NONE, S.FIT
TILE = WP.SCATTER_TILE
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]           # around a wave, a workgroup and the tile
SCATTER_CONTENTS = ["identity", "reverse", "onto-one", "every-other", "first", "last", "2d-dim0", "2d-dim1", "partial"]
COMPLEMENT_CONTENTS = ["none", "all", "evens", "prefix", "suffix", "outside"]
ONEHOT_CLASSES = [1, 2, 65]


class IndexedBuilder(S.Builder):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.unwritten = []                        # the cells that must stay zero

    def scatter(self, dst, base, index, src, extent, mult, offsets):
        """a SCATTER record: element j goes to s_j * mult + offsets[j]; a later element overwrites an earlier one -> Cells of the tensor"""
        dst, offsets = list(dst), list(offsets)
        m = len(index)
        assert len(dst) == len(base) and len(src) == m == len(offsets) and m >= 1
        out = list(self._read(base))
        bad = []
        for j, (v, x, off) in enumerate(zip(self._read(index), self._read(src), offsets)):
            s = S.signed(v)
            if s < 0 or s >= extent or abs(s) >= FIT:
                bad.append(j)
            else:
                out[s * mult + off] = x
        ri = len(self.records)
        self.records.append([WP.SCATTER, len(dst), m, mult, self._push(dst), self._push(base.idx), self._push([extent] + index.idx + src.idx + offsets), 0])
        for c, v in zip(dst, out):
            assert c not in self.expect, "cell %d is planted twice" % c
            self.expect[c] = 0 if bad else v
        self.refused += [(ri, j, None) for j in bad]
        if bad:
            self.unwritten += dst
        self.n_cells += len(dst)
        return S.Cells(dst, [None] * len(dst) if bad else out)

    def complement(self, dst, src, n):
        """a COMPLEMENT record over {0 .. n - 1}: the positions no source names, ascending, as many as there are destinations"""
        dst = list(dst)
        assert len(dst) == n - len(src)
        want = sorted(set(range(n)) - {S.signed(v) for v in self._read(src)})[:len(dst)]
        assert len(want) == len(dst)
        self.records.append([WP.COMPLEMENT, len(dst), n, len(src), self._push(dst), self._push(src.idx), 0, 0])
        for c, v in zip(dst, want):
            assert c not in self.expect, "cell %d is planted twice" % c
            self.expect[c] = v
        self.n_cells += len(dst)
        return S.Cells(dst, want)

    def onehot(self, dst, index, positions, classes):
        """a ONEHOT record: lane e is 1 when the index it reads equals positions[e]; an index outside [0, classes) is refused"""
        vals = [None if not 0 <= S.signed(v) < classes else int(S.signed(v) == p) for v, p in zip(self._read(index), positions)]
        out = self._elem(WP.ONEHOT, dst, index.idx, vals, list(positions), p0=classes)
        self.unwritten += [c for c, v in zip(out.idx, out.val) if v is None]
        return out


class IndexedCase(S.Case):
    def __init__(self, b, outputs=()):
        super().__init__(b, outputs)
        self.unwritten = list(b.unwritten)


def _builder(total):
    """a geometry with room for `total` cells along the linear coordinate"""
    k = min(max(6, (total - 1).bit_length() - 3), 14)
    n_advice = -(-(total + 4) >> k) + 1
    assert n_advice <= 64
    return IndexedBuilder(k, n_advice)


def scatter_elements(name, n, rng):
    """(index values, extent, mult, offsets) of `name` on a tensor of n cells"""
    if name == "identity":
        return list(range(n)), n, 1, [0] * n
    if name == "reverse":
        return list(range(n - 1, -1, -1)), n, 1, [0] * n
    if name == "onto-one":                                             # n + 3 elements on one target: the last wins
        t = rng.randrange(n)
        return [t] * (n + 3), n, 1, [0] * (n + 3)
    if name == "every-other":
        idx = list(range(0, n, 2))
        return idx, n, 1, [0] * len(idx)
    if name == "first":
        return [0], n, 1, [0]
    if name == "last":
        return [n - 1], n, 1, [0]
    C = 3 if n >= 3 else 1
    rows = n // C
    if name == "2d-dim0":                                              # an m x C index into a rows x C tensor along dim 0: mult = C, offset = the column
        m = rng.randrange(1, rows + 1)
        cols = [rng.sample(range(rows), m) for _ in range(C)]          # distinct in every column
        return [cols[c][i] for i in range(m) for c in range(C)], rows, C, [c for _ in range(m) for c in range(C)]
    if name == "2d-dim1":                                              # a rows x m index along dim 1: mult = 1, offset = row * C
        m = rng.randrange(1, C + 1)
        return [s for _ in range(rows) for s in rng.sample(range(C), m)], C, 1, [r * C for r in range(rows) for _ in range(m)]
    m = rng.randrange(1, n + 1)                                        # a random partial permutation
    return rng.sample(range(n), m), n, 1, [0] * m


def scatter_case(n, seed, contents=SCATTER_CONTENTS):
    """one plan: a base of n inputs, and per content its index and source inputs and a SCATTER record of n cells"""
    rng = random.Random(7919 * seed + n)
    specs = [scatter_elements(name, n, rng) for name in contents]
    b = _builder(n + len(specs) * (2 * (n + 3) + n))                   # room for the most elements a content has: the same columns for every seed
    base = b.input(b.fresh(n, corner=True), [rng.randrange(-1000, 1000) for _ in range(n)])
    outs = []
    for idx, extent, mult, offsets in specs:
        index = b.input(b.fresh(len(idx)), idx)
        src = b.input(b.fresh(len(idx)), [rng.randrange(1 << 40, 1 << 41) * rng.choice((-1, 1)) for _ in idx])
        cells = b.fresh(n, corner=True)
        rng.shuffle(cells)
        outs.append(b.scatter(cells, base, index, src, extent, mult, offsets))
    assert not b.refused and not b.unwritten
    return IndexedCase(b, [o.idx[0] for o in outs] + [outs[0].idx[-1]])


def complement_sources(name, n):
    if name == "none":
        return []
    if name == "all":
        return list(range(n))
    if name == "evens":
        return list(range(0, n, 2))
    if name == "prefix":
        return list(range(n // 3))
    if name == "suffix":
        return list(range(n - n // 3, n))
    return [0, 0, -1, n, FIT, -FIT, n // 2, n // 2][:n]               # duplicates and values outside the set remove nothing twice: the truncation shows


def complement_case(n, seed):
    rng = random.Random(104729 * seed + n)
    specs = [complement_sources(name, n) for name in COMPLEMENT_CONTENTS]
    b = _builder(sum(n for _ in specs) + 8)
    outs = []
    for vals in specs:
        vals = list(vals)
        rng.shuffle(vals)
        src = b.input(b.fresh(len(vals)), vals) if vals else S.Cells([], [])
        cells = b.fresh(n - len(vals))
        rng.shuffle(cells)
        outs.append(b.complement(cells, src, n))
    return IndexedCase(b, [o.idx[0] for o in outs if len(o)] + [o.idx[-1] for o in outs if len(o)])


def onehot_case(seed, outside=False):
    """classes 1, 2 and 65, each at its first and last index, every position; `outside`: also the indices -1, classes and +-2^62"""
    rng = random.Random(seed)
    b = _builder(2048)
    outs = []
    for classes in ONEHOT_CLASSES:
        idx = sorted({0, classes - 1}) + ([-1, classes, FIT, -FIT] if outside else [])
        rng.shuffle(idx)
        index = b.input(b.fresh(len(idx), corner=True), idx)
        lanes = [(i, p) for i in range(len(idx)) for p in range(classes)]
        rng.shuffle(lanes)
        outs.append(b.onehot(b.fresh(len(lanes)), index.take([i for i, _ in lanes]), [p for _, p in lanes], classes))
    return IndexedCase(b, [] if outside else [o.idx[0] for o in outs])


def offsets_case(seed):
    """a complement over 256 tiles and one position more: the workgroup that turns the tiles' counts into offsets makes a second round.  500
    seeded sources, which may repeat, and the last 300 positions"""
    n = 256 * TILE + 1
    rng = random.Random(seed)
    vals = [rng.randrange(n) for _ in range(500)] + list(range(n - 300, n))
    b = IndexedBuilder(17, 10)
    src = b.input(b.fresh(len(vals)), vals)
    out = b.complement(b.fresh(n - len(vals)), src, n)
    return IndexedCase(b, [out.idx[0], out.idx[-1]])


BAD_AT = (3, 70)                                                       # the offending elements of the middle scatter


def failing_case(n, bad, seed=0):
    """three identity-shaped scatters of n elements onto one base; with `bad` elements 3 and 70 of the middle one hold the indices n (the extent)
    and -1.  The plan is the same either way and for every seed: only the inputs follow them."""
    assert n > max(BAD_AT)
    rng = random.Random(seed)
    b = _builder(n + 3 * 3 * n)
    base = b.input(b.fresh(n), [rng.randrange(-50, 51) for _ in range(n)])
    outs = []
    for r in range(3):
        idx = list(range(n))
        rng.shuffle(idx)
        if bad and r == 1:
            idx[BAD_AT[0]], idx[BAD_AT[1]] = n, -1
        index = b.input(b.fresh(n), idx)
        src = b.input(b.fresh(n), [rng.randrange(-50, 51) for _ in range(n)])
        outs.append(b.scatter(b.fresh(n), base, index, src, n, 1, [0] * n))
    return IndexedCase(b, [outs[0].idx[0], outs[2].idx[n - 1]])


def _scatter(n): return lambda seed: scatter_case(n, seed)
def _complement(n): return lambda seed: complement_case(n, seed)


CASES = {}
for _n in SIZES:
    CASES["scatter-n%d" % _n] = _scatter(_n)
    CASES["complement-n%d" % _n] = _complement(_n)
CASES["onehot-edges"] = lambda seed: onehot_case(seed)
CASES["onehot-outside"] = lambda seed: onehot_case(seed, outside=True)


# ---- what the validators refuse ---------------------------------------------------------------------------------------------------------------
def small_plan():
    """0 INPUT (a base of six), 1 INPUT (two indices), 2 INPUT (two sources), 3 SCATTER of a 3 x 2 tensor along dim 0 (extent 3, mult 2, offsets
    0 and 1), 4 COMPLEMENT of the two indices in {0 .. 5}, 5 ONEHOT of index 0 over three classes"""
    b = IndexedBuilder(4, 3)
    base = b.input(b.rows(0, range(6)), [1, 2, 3, 4, 5, 6])
    index = b.input(b.rows(0, range(6, 8)), [2, 0])
    src = b.input(b.rows(0, range(8, 10)), [10, 20])
    t = b.scatter(b.rows(1, range(6)), base, index, src, 3, 2, [0, 1])
    c = b.complement(b.rows(2, range(4)), index, 6)
    h = b.onehot(b.rows(2, range(4, 7)), index.take([1, 1, 1]), [0, 1, 2], 3)
    return IndexedCase(b, t.idx + c.idx + h.idx)


def _tampered(plan):
    q = WP.WitnessPlan.from_bytes(plan.to_bytes())
    q.records, q.pool = q.records.copy(), q.pool.copy()
    return q


def bad_plans():
    """(the words both validators must use, the record they must name, a plan with that one defect)"""
    plan = small_plan().plan
    COUNT, P0, P1, DST, A, B = 1, 2, 3, 4, 5, 6
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
    words = len(plan.pool)
    unwritten = (2 << plan.k) + 15
    # SCATTER (record 3): b -> extent, 2 index cells, 2 source cells, 2 offsets
    sb = rec[3][B]
    bad("bad scatter shape", 3, P0, 0)
    bad("bad scatter shape", 3, P1, 0)
    bad("bad scatter shape", 3, pool_at=sb, pool_value=0)              # a zero extent
    bad("bad scatter shape", 3, COUNT, (1 << 28) + 1)
    bad("bad scatter shape", 3, P0, words)                             # 1 + 3m words past the pool
    bad("bad scatter shape", 3, B, words - 6)
    bad("bad scatter shape", 3, B, NONE)
    bad("bad scatter shape", 3, A, words - 5)
    bad("bad scatter shape", 3, DST, words + 1)
    bad("bad scatter shape", 3, pool_at=sb, pool_value=4)              # extent 4: 1 + 3 * 2 = 7 >= 6
    bad("bad scatter shape", 3, P1, 3)                                 # mult 3: 1 + 2 * 3 = 7 >= 6
    bad("bad scatter shape", 3, pool_at=sb + 6, pool_value=2)          # offset 2: 2 + 2 * 2 = 6 >= 6
    bad("bad scatter shape", 3, pool_at=sb + 5, pool_value=NONE)
    bad("a cell is read before an earlier record has written it", 3, pool_at=sb + 1, pool_value=unwritten)       # an index cell
    bad("a cell is read before an earlier record has written it", 3, pool_at=sb + 4, pool_value=unwritten)       # a source cell
    bad("a cell is read before an earlier record has written it", 3, pool_at=rec[3][A] + 2, pool_value=plan.pool[rec[3][DST]])      # its own destination as a base
    bad("cell index out of range", 3, pool_at=sb + 2, pool_value=cells)
    bad("cell index out of range", 3, pool_at=rec[3][A], pool_value=cells)
    bad("cell index out of range", 3, pool_at=rec[3][DST] + 5, pool_value=cells)
    bad("a cell is written twice", 3, pool_at=rec[3][DST] + 1, pool_value=plan.pool[rec[3][DST]])
    bad("a cell is written twice", 3, pool_at=rec[3][DST], pool_value=plan.pool[rec[0][DST]])
    # COMPLEMENT (record 4)
    bad("bad complement shape", 4, P1, 7)                              # more sources than the set holds
    bad("bad complement shape", 4, P1, 1)                              # count != n - m
    bad("bad complement shape", 4, COUNT, 5)
    bad("bad complement shape", 4, P0, 7)
    bad("bad complement shape", 4, P0, (1 << 28) + 1)
    bad("bad complement shape", 4, A, words - 1)
    bad("bad complement shape", 4, A, NONE)
    bad("bad complement shape", 4, DST, words - 3)
    bad("a cell is read before an earlier record has written it", 4, pool_at=rec[4][A] + 1, pool_value=unwritten)
    bad("cell index out of range", 4, pool_at=rec[4][DST] + 3, pool_value=cells)
    bad("a cell is written twice", 4, pool_at=rec[4][DST] + 3, pool_value=plan.pool[rec[3][DST]])
    # ONEHOT (record 5)
    bad("zero one-hot classes", 5, P0, 0)
    bad("a cell is read before an earlier record has written it", 5, pool_at=rec[5][A], pool_value=unwritten)
    bad("cell index out of range", 5, pool_at=rec[5][A] + 2, pool_value=cells)
    bad("a cell is written twice", 5, pool_at=rec[5][DST], pool_value=plan.pool[rec[4][DST]])
    return out
