"""Synthetic plans for the ARGEXT record kind with their expected cells in closed form, and the plans both validators must refuse.

`ArgBuilder` is tests/witness_synth.py's `Builder` (imported, left as it is) with one method for an ARGEXT record.  The expectation is
worked out from the planted values alone: `max(range(n), key=lambda j: (s[j], -j))` for mode 0 and `min(range(n), key=lambda j: (s[j], j))`
for mode 1 -- the reference's `max_by_key` / `min_by_key`; nothing here decodes a pool or walks a record list, so it shares no code with
`witness_plan.run_plan_host` or with the kernels.  A segment that holds a source beyond 62 bits is expected to leave its cell unwritten:
it stays zero and is listed in `unwritten`; the offending SOURCE elements are listed in `refused`.  `CASES` maps a test id to
`make(seed) -> ArgCase`; tests/test_witness_plan_pool_cpu.py holds the host interpreter to the closed form, tests/test_gpu_witness_pool.py
the device columns.  `bad_plans()` lists (the words of the refusal, the record, a plan with that one defect)."""
import random

import witness_synth as S
from ezkl_amd import witness_plan as WP

R, NONE, FIT = S.R, S.NONE, S.FIT
CHUNK = WP.ARGEXT_CHUNK
LENGTHS = [1, 2, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]     # around a wave, a workgroup and a chunk
MANY = [(300, 5), (7, 64), (9, 100), (130, 1)]                         # segments x length
CONTENTS = ["equal", "ascending", "descending", "last", "tie63", "tie4095", "edges", "negative", "random"]


def closed_form(seg, mode):
    return min(range(len(seg)), key=lambda j: (seg[j], j)) if mode else max(range(len(seg)), key=lambda j: (seg[j], -j))


class ArgBuilder(S.Builder):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.unwritten = []                        # the cells of the segments that must stay zero

    def argext(self, dst, src, n, mode):
        """an ARGEXT record over the cells `src` in segments of n -> Cells of the positions"""
        vals = [S.signed(v) for v in self._read(src)]
        dst = list(dst)
        assert len(src) == n * len(dst)
        ri = len(self.records)
        self.records.append([WP.ARGEXT, len(dst), n, mode, self._push(dst), self._push(src.idx), 0, 0])
        want = []
        for g, c in enumerate(dst):
            seg = vals[g * n:(g + 1) * n]
            bad = [g * n + j for j, s in enumerate(seg) if abs(s) >= FIT]
            assert c not in self.expect, "cell %d is planted twice" % c
            want.append(None if bad else closed_form(seg, mode))
            self.expect[c] = want[-1] or 0
            self.refused += [(ri, e, c) for e in bad]               # (c is the refused segment's cell: it must stay zero)
            if bad:
                self.unwritten.append(c)
        self.n_cells += len(dst)
        return S.Cells(dst, want)


class ArgCase(S.Case):
    def __init__(self, b, outputs=()):
        super().__init__(b, outputs)
        self.unwritten = list(b.unwritten)


def content(name, n, mode, rng):
    """n signed values below 2^62 in magnitude; "the extremum" is the greatest value for mode 0, the least for mode 1"""
    sgn = -1 if mode else 1
    if name == "equal":
        return [rng.choice([0, -1, 7, -(FIT - 1), FIT - 1])] * n
    if name == "ascending":
        start = rng.randrange(-n, n)
        return [start + i for i in range(n)]
    if name == "descending":
        start = rng.randrange(-n, n)
        return [start - i for i in range(n)]
    if name == "last":                                                # the extremum only in the last position
        return [sgn * rng.randrange(-5, 3) for _ in range(n - 1)] + [sgn * 3]
    if name in ("tie63", "tie4095"):                                  # two equal extrema side by side across a wave / a chunk: the first wins
        at = 63 if name == "tie63" else CHUNK - 1
        vals = [sgn * rng.randrange(-9, 0) for _ in range(n)]
        for j in (at, at + 1):
            if j < n:
                vals[j] = sgn * 4
        return vals
    if name == "edges":                                               # +-(2^62 - 1) next to 0 and -1
        cycle = [0, FIT - 1, -1, -(FIT - 1), 0, FIT - 1, -1, -(FIT - 1)]
        at = rng.randrange(len(cycle))
        return [cycle[(at + i) % len(cycle)] for i in range(n)]
    if name == "negative":
        return [-rng.randrange(1, 50) for _ in range(n)]
    return [rng.randrange(-3, 4) for _ in range(n)]                   # many ties


def _geometry(total):
    """k such that one column holds `total` cells: sources in column 0, positions in column 1"""
    return max(4, (total - 1).bit_length())


def arg_case(segments, mode, seed):
    """segments: [(content name, n)] of one length n.  The sources are inputs in column 0, read through a seeded permutation of its rows; the
    destinations are a seeded choice of the rows of column 1"""
    n = segments[0][1]
    assert all(m == n for _, m in segments)
    total = n * len(segments)
    rng = random.Random(1000 * seed + total + mode)
    vals = [v for name, _ in segments for v in content(name, n, mode, rng)]
    k = _geometry(total)
    b = ArgBuilder(k, 2)
    src = b.input(b.rows(0, rng.sample(range(1 << k), total)), vals)
    pos = b.argext(b.rows(1, rng.sample(range(1 << k), len(segments))), src, n, mode)
    assert not b.refused and not b.unwritten
    return ArgCase(b, [pos.idx[0], pos.idx[-1]])


BAD_AT = (63, 64)                                                      # the offending elements of the middle segment: 2^62 and -2^62


def failing_case(n, bad, seed=0):
    """three segments of n over column 0; with `bad` the middle one holds 2^62 at element 63 and -2^62 at element 64.  Mode n % 2.  The plan
    is the same either way and for every seed: only the inputs follow them."""
    assert n > max(BAD_AT)
    rng = random.Random(seed)
    vals = [rng.randrange(-50, 51) for _ in range(3 * n)]
    if bad:
        vals[n + BAD_AT[0]], vals[n + BAD_AT[1]] = FIT, -FIT
    k = _geometry(3 * n)
    b = ArgBuilder(k, 2)
    src = b.input(b.rows(0, range(3 * n)), vals)
    pos = b.argext(b.rows(1, [5, 0, 9]), src, n, n % 2)
    return ArgCase(b, [pos.idx[0], pos.idx[2]])


def _case(segments, mode): return lambda seed: arg_case(segments, mode, seed)


CASES = {}
for _mode in (0, 1):
    for _n in LENGTHS:
        CASES["argext-n%d-mode%d" % (_n, _mode)] = _case([(c, _n) for c in CONTENTS], _mode)
    for _segs, _n in MANY:
        CASES["argext-%dx%d-mode%d" % (_segs, _n, _mode)] = _case([(CONTENTS[i % len(CONTENTS)], _n) for i in range(_segs)], _mode)


# ---- what the validators refuse ---------------------------------------------------------------------------------------------------------------
def small_plan():
    """0 CONST (eight values), 1 ARGEXT over them in two segments of four, argmin"""
    b = ArgBuilder(4, 2)
    src = b.const(b.rows(0, range(8)), [v % R for v in (5, -2, 5, -2, 3, 3, -7, 9)])
    pos = b.argext(b.rows(1, range(2)), src, 4, 1)
    return ArgCase(b, pos.idx)


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
    words = len(plan.pool)
    bad("bad arg-extremum shape", 1, P0, 0)                            # n = 0
    bad("bad arg-extremum shape", 1, P1, 2)                            # a mode above 1
    bad("bad arg-extremum shape", 1, P1, NONE)
    bad("bad arg-extremum shape", 1, P0, (1 << 27) + 1)                # 2 segments: beyond 2^28 sources
    bad("bad arg-extremum shape", 1, COUNT, (1 << 26) + 1)             # segments of 4: beyond 2^28 sources
    bad("bad arg-extremum shape", 1, P0, 5)                            # ten sources where the pool has eight left
    bad("bad arg-extremum shape", 1, COUNT, 3)                         # a third segment past the pool
    bad("bad arg-extremum shape", 1, A, words - 7)
    bad("bad arg-extremum shape", 1, A, words + 1)
    bad("bad arg-extremum shape", 1, DST, words - 1)
    bad("bad arg-extremum shape", 1, DST, NONE)
    unwritten = (1 << plan.k) + 15
    bad("a cell is read before an earlier record has written it", 1, pool_at=rec[1][A] + 3, pool_value=unwritten)
    bad("a cell is read before an earlier record has written it", 1, pool_at=rec[1][A], pool_value=plan.pool[rec[1][DST]])      # ... its own destination
    bad("cell index out of range", 1, pool_at=rec[1][A], pool_value=cells)
    bad("cell index out of range", 1, pool_at=rec[1][DST] + 1, pool_value=cells)
    bad("a cell is written twice", 1, pool_at=rec[1][DST] + 1, pool_value=plan.pool[rec[1][DST]])
    bad("a cell is written twice", 1, pool_at=rec[1][DST], pool_value=plan.pool[rec[0][DST]])
    return out
