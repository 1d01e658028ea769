"""Synthetic plans for the SORT and ARGSORT record kinds with their expected cells in closed form, and the plans both validators must
refuse.

`SortBuilder` is tests/witness_synth.py's `Builder` (imported, left as it is) with one method for a SORT / ARGSORT pair over the same
source cells.  The expectation is worked out from the planted values alone, by RANK: element j of a segment, with signed value s, goes to
place (the number of elements below s) + (the number of elements equal to s before j -- after j for mode 1); nothing here calls a sort
on (value, position) pairs, decodes a pool or walks a record list, so it shares no code with `witness_plan.run_plan_host` or with the
kernels.  A segment that holds a key beyond 62 bits is expected to write none of its cells: they stay zero and are listed in
`unwritten`; the offending SOURCE elements are listed in `refused`, once per record.  `CASES` maps a test id to `make(seed) -> SortCase`;
tests/test_witness_plan_sort_cpu.py holds the host interpreter to the closed form, tests/test_gpu_witness_sort.py the device columns.
`bad_plans()` lists (the words of the refusal, the record, a plan with that one defect)."""
import random
from collections import Counter

import witness_synth as S
from ezkl_amd import witness_plan as WP

R, NONE, FIT = S.R, S.NONE, S.FIT
TILE = WP.SORT_TILE
LENGTHS = [1, 2, 3, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 5]     # below, at and above a wave and the tile; two tiles plus padding
CONTENTS = ["equal", "two", "ascending", "descending", "edges", "random"]


def ranks(signed_vals, mode):
    """place of each element in the order by (value, position), the position descending among equals for mode 1"""
    below, run = {}, 0
    count = Counter(signed_vals)
    for v in sorted(count):
        below[v] = run
        run += count[v]
    seen, out = Counter(), []
    for s in signed_vals:
        out.append(below[s] + (count[s] - 1 - seen[s] if mode else seen[s]))
        seen[s] += 1
    return out


class SortBuilder(S.Builder):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.unwritten = []                        # the cells of the segments that must stay zero

    def sort_pair(self, dst_sorted, dst_index, src, n, mode):
        """a SORT record then an ARGSORT record over the cells `src`, in segments of n -> (Cells of the sorted values, Cells of the positions)"""
        vals = [S.signed(v) for v in self._read(src)]
        assert len(src) % n == 0 and len(dst_sorted) == len(dst_index) == len(src)
        want = {WP.SORT: [None] * len(src), WP.ARGSORT: [None] * len(src)}
        bad = [e for e, s in enumerate(vals) if abs(s) >= FIT]
        for g in range(0, len(src), n):
            seg = vals[g:g + n]
            if any(abs(s) >= FIT for s in seg):
                continue
            for j, place in enumerate(ranks(seg, mode)):
                want[WP.SORT][g + place], want[WP.ARGSORT][g + place] = seg[j] % R, j
        out = []
        for kind, dst in ((WP.SORT, list(dst_sorted)), (WP.ARGSORT, list(dst_index))):
            ri = len(self.records)
            self.records.append([kind, len(dst), n, mode, self._push(dst), self._push(src.idx), 0, 0])
            for c, v in zip(dst, want[kind]):
                assert c not in self.expect, "cell %d is planted twice" % c
                self.expect[c] = 0 if v is None else v
                if v is None:
                    self.unwritten.append(c)
            self.refused += [(ri, e, dst[e]) for e in bad]          # (dst[e] lies in the refused segment: it must stay zero)
            self.n_cells += len(dst)
            out.append(S.Cells(dst, want[kind]))
        return out


class SortCase(S.Case):
    def __init__(self, b, outputs=()):
        super().__init__(b, outputs)
        self.unwritten = list(b.unwritten)


def content(name, n, rng):
    """n signed values below 2^62 in magnitude"""
    if name == "equal":
        return [rng.choice([0, -1, 7, -(FIT - 1), FIT - 1])] * n
    if name == "two":
        lo = rng.choice([-3, 0, -(FIT - 1)])
        hi = lo + rng.choice([1, 5])
        return [rng.choice([lo, hi]) for _ in range(n)]
    if name == "ascending":
        start = rng.randrange(-n, n)
        return [start + i for i in range(n)]
    if name == "descending":
        start = rng.randrange(-n, n)
        return [start - i for i in range(n)]
    if name == "edges":                                              # +-(2^62 - 1) next to 0 and -1
        cycle = [FIT - 1, 0, -1, -(FIT - 1), 0, FIT - 1, -1, -(FIT - 1)]
        at = rng.randrange(len(cycle))
        return [cycle[(at + i) % len(cycle)] for i in range(n)]
    return [rng.randrange(-4, 5) for _ in range(n)]                   # duplicates of every value


def _geometry(total):
    """k such that one column holds `total` cells: sources in column 0, sorted values in column 1, positions in column 2"""
    return max(4, (total - 1).bit_length())


def sort_case(segments, mode, seed):
    """segments: [(content name, n)] of one length n.  The sources are inputs in column 0, read through a seeded permutation of its
    rows; the destinations are seeded permutations of the rows of columns 1 and 2 (row 0 and the last row among them when they fit)"""
    n = segments[0][1]
    assert all(m == n for _, m in segments)
    total = n * len(segments)
    rng = random.Random(1000 * seed + total + mode)
    vals = [v for name, _ in segments for v in content(name, n, rng)]
    k = _geometry(total)
    b = SortBuilder(k, 3)
    rows = lambda col: b.rows(col, rng.sample(range(1 << k), total))
    src = b.input(rows(0), vals)
    srt, idx = b.sort_pair(rows(1), rows(2), src, n, mode)
    assert not b.refused and not b.unwritten
    return SortCase(b, [srt.idx[0], srt.idx[-1], idx.idx[0], idx.idx[-1]])


BAD_AT = (5, 40, 41)                                                   # the offending elements of the middle segment: 2^62, -2^62, 2^190


def failing_case(n, bad, seed=0):
    """three segments of n over column 0; with `bad` the middle one holds 2^62 and -2^62 (inputs) and 2^190 (the product of an input flag
    and a constant: high limbs set).  Mode n % 2.  The plan is the same either way and for every seed: only the inputs follow them."""
    assert n > max(BAD_AT)
    rng = random.Random(seed)
    vals = [rng.randrange(-50, 51) for _ in range(3 * n)]
    flag = 0
    if bad:
        vals[n + BAD_AT[0]], vals[n + BAD_AT[1]], flag = FIT, -FIT, 1
    k = _geometry(3 * n + 2)
    b = SortBuilder(k, 4)
    at = n + BAD_AT[2]
    inp = b.input(b.rows(0, [r for r in range(3 * n) if r != at]), [v for e, v in enumerate(vals) if e != at])
    big = b.const([b.cell(3, 0)], [1 << 190])
    f = b.input([b.cell(3, 1)], [flag])
    prod = b.mul([b.cell(0, at)], f, big)
    src = S.Cells(inp.idx[:at] + prod.idx + inp.idx[at:], inp.val[:at] + prod.val + inp.val[at:])
    srt, idx = b.sort_pair(b.rows(1, range(3 * n)), b.rows(2, range(3 * n - 1, -1, -1)), src, n, n % 2)
    return SortCase(b, [srt.idx[0], idx.idx[3 * n - 1]])


def _case(segments, mode): return lambda seed: sort_case(segments, mode, seed)


CASES = {}
for _mode in (0, 1):
    for _n in LENGTHS:
        CASES["sort-n%d-mode%d" % (_n, _mode)] = _case([(c, _n) for c in CONTENTS], _mode)
    for _n in (1, 3, TILE + 1):                                        # a record of one segment
        CASES["sort-single-n%d-mode%d" % (_n, _mode)] = _case([("random", _n)], _mode)
    CASES["sort-9x100-mode%d" % _mode] = _case([(CONTENTS[i % len(CONTENTS)], 100) for i in range(9)], _mode)      # P = 128: 16 to a tile
    CASES["sort-300x5-mode%d" % _mode] = _case([(CONTENTS[i % len(CONTENTS)], 5) for i in range(300)], _mode)      # P = 8: 256 to a tile, a ragged second one


# ---- what the validators refuse ---------------------------------------------------------------------------------------------------------------
def small_plan():
    """0 CONST (eight values), 1 SORT and 2 ARGSORT over them in two segments of four"""
    b = SortBuilder(4, 3)
    src = b.const(b.rows(0, range(8)), [v % R for v in (5, -2, 5, 0, 3, 3, -7, 9)])
    srt, idx = b.sort_pair(b.rows(1, range(8)), b.rows(2, range(8)), src, 4, 1)
    return SortCase(b, [srt.idx[0], idx.idx[0]])


def _tampered(plan):
    q = WP.WitnessPlan.from_bytes(plan.to_bytes())
    q.records, q.pool = q.records.copy(), q.pool.copy()
    return q


def bad_plans():
    """(the words both validators must use, the record they must name, a plan with that one defect)"""
    plan = small_plan().plan
    COUNT, P0, P1, DST, A = 1, 2, 3, 4, 5
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
    for r in (1, 2):
        bad("bad sort shape", r, P0, 0)                             # n = 0
        bad("bad sort shape", r, P0, 3)                             # 8 % 3 != 0
        bad("bad sort shape", r, P0, 16)                            # a segment longer than the record
        bad("bad sort shape", r, P1, 2)                             # a mode above 1
        bad("bad sort shape", r, P1, NONE)
        bad("bad sort shape", r, COUNT, (1 << 28) + 4)              # whole segments, beyond 2^28 cells
        bad("bad sort shape", r, COUNT, 7)
    unwritten = (2 << plan.k) + 15
    bad("a cell is read before an earlier record has written it", 1, pool_at=rec[1][A] + 3, pool_value=unwritten)
    bad("a cell is read before an earlier record has written it", 2, pool_at=rec[2][A], pool_value=plan.pool[rec[2][DST]])      # ... its own destination
    bad("cell index out of range", 1, pool_at=rec[1][A], pool_value=cells)
    bad("cell index out of range", 2, pool_at=rec[2][DST] + 7, pool_value=cells)
    bad("a cell is written twice", 1, pool_at=rec[1][DST] + 1, pool_value=plan.pool[rec[1][DST]])
    bad("a cell is written twice", 2, pool_at=rec[2][DST], pool_value=plan.pool[rec[1][DST]])
    bad("a cell is written twice", 1, pool_at=rec[1][DST], pool_value=plan.pool[rec[0][DST]])
    return out
