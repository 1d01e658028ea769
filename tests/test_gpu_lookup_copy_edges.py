"""The lookup, copy-check and streaming kernels of csrc/vecops.hip on structured inputs: collision chains in the multiplicity hash table
(also wrapping past its last slot, and two chains running into each other), equal table rows racing for "first row wins", runs of equal
rows at wave and workgroup boundaries, chosen numbers of distinct targets per wave of the count pass, every `usable` edge, the record
cap of the mock prover's reports inside a wave's run of slots, the accumulated missing counter, and every grid-stride loop past its
first pass.  Expected values come from tests/lookup_edge_ref.py (dicts and sets over the stored bytes) and from oracle.binding; every
comparison is word for word or set equality."""
import ctypes as C
import functools

import numpy as np
import pytest

import lookup_edge_ref as ER
from conftest import R, fe_from_int, rand_fr
from oracle import binding as ob

pytestmark = pytest.mark.gpu
GUARD = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def B(hip):
    from ezkl_amd import backend
    return backend


def _dev(B, arrays):
    return [B.DeviceBuffer.from_numpy(a) for a in arrays]


def _column(buf, n):
    return buf.to_numpy(shape=(n, 4))


# ---- the report entry points on a caller's record buffer with guard records around it ---------------------------------------------------
def _guarded(B, cap):
    """(buffer, pointer to `cap` records): one guard record in front, eight behind, everything 0xA5"""
    buf = B.DeviceBuffer.from_numpy(np.full(2 * (1 + cap + 8), GUARD, np.uint64))
    return buf, buf.ptr + 16


def _read_guarded(buf, cap, counters):
    """(records written, counters) after checking that nothing but the first min(cap, total) records changed"""
    words = buf.to_numpy(np.uint64).reshape(-1, 2)
    cnt = [int(x) for x in counters.to_numpy(np.uint64)]
    m = min(cap, cnt[0])
    assert (words[0] == GUARD).all() and (words[1 + m:] == GUARD).all()
    rec = words[1:1 + m].copy().view(np.uint32).reshape(m, 4)
    return [tuple(int(x) for x in r) for r in rec], cnt


def _miss_rows(B, flat, which, table_ptrs, n_rows, usable, cap):
    from ezkl_amd import lib as L
    buf, rec = _guarded(B, cap)
    cnt = B.DeviceBuffer.from_numpy(np.zeros(1 + len(table_ptrs), np.uint64))
    a_in = (C.c_void_p * max(1, len(flat)))(*flat)
    a_which = (C.c_uint32 * max(1, len(which)))(*which)
    a_tab = (C.c_void_p * len(table_ptrs))(*table_ptrs)
    L.check(L.load().ezkl_hip_lookup_missing_rows_dev(a_in, a_which, C.c_uint32(len(flat)), a_tab, C.c_uint32(len(table_ptrs)), C.c_uint32(n_rows),
                                                      C.c_uint32(usable), C.c_void_p(rec), C.c_uint32(cap), C.c_void_p(cnt.ptr), C.c_void_p(None)),
            "ezkl_hip_lookup_missing_rows_dev")
    return _read_guarded(buf, cap, cnt)


def _copy_check(B, col_ptrs, next_ptr, log_n, cap):
    from ezkl_amd import lib as L
    buf, rec = _guarded(B, cap)
    cnt = B.DeviceBuffer.from_numpy(np.zeros(1, np.uint64))
    a = (C.c_void_p * len(col_ptrs))(*col_ptrs)
    L.check(L.load().ezkl_hip_copy_check_dev(a, C.c_uint32(len(col_ptrs)), C.c_void_p(next_ptr), C.c_uint32(log_n), C.c_void_p(rec), C.c_uint32(cap),
                                             C.c_void_p(cnt.ptr), C.c_void_p(None)), "ezkl_hip_copy_check_dev")
    return _read_guarded(buf, cap, cnt)


# ---- one lookup argument through the three entry points -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _filler(n_rows, usable):
    """two ordinary arguments (1 and 2 inputs, 3 missing values) that share a batch with the argument under test, and their reference"""
    rng = np.random.default_rng(7000 + 31 * n_rows + usable)
    tables = [rand_fr(rng, n_rows)[rng.integers(0, max(2, n_rows // 3), n_rows)] for _ in range(2)]
    inputs = [[t[rng.integers(0, max(1, usable), n_rows)] for _ in range(q)] for t, q in zip(tables, (1, 2))]
    inputs[0][0][0], inputs[1][1][max(1, usable) - 1], inputs[1][0][n_rows // 2] = rand_fr(rng, 3)
    ref = [ER.multiplicity(t, ins, n_rows, usable) for t, ins in zip(tables, inputs)]
    for a in tables + inputs[0] + inputs[1]:
        a.setflags(write=False)
    return tables, inputs, [ER.counts_to_fr(c) for c, _ in ref], sum(m for _, m in ref)


def _check_lookup(B, table, inputs, n_rows, usable):
    """lookup_multiplicity, the same argument in the middle of a lookup_multiplicity_batch of three, and lookup_missing_rows, each
    against the reference (and so with each other).  Returns the reference (counts, missing)."""
    counts, missing = ER.multiplicity(table, inputs, n_rows, usable)
    want = ER.counts_to_fr(counts)
    dt, di = _dev(B, [table])[0], _dev(B, inputs)
    ptrs = [d.ptr for d in di]
    m_one, miss_one = B.lookup_multiplicity(ptrs, dt.ptr, n_rows, usable)
    got = _column(m_one, n_rows)
    assert miss_one == missing
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:8]

    f_tables, f_inputs, f_want, f_missing = _filler(n_rows, usable)
    ft, fi = _dev(B, f_tables), [_dev(B, ins) for ins in f_inputs]
    outs, total = B.lookup_multiplicity_batch([[d.ptr for d in fi[0]], ptrs, [d.ptr for d in fi[1]]], [ft[0].ptr, dt.ptr, ft[1].ptr], n_rows, usable)
    assert total == missing + f_missing
    for o, w in zip(outs, (f_want[0], want, f_want[1])):
        assert (_column(o, n_rows) == w).all()

    ref = ER.miss_records([table], [inputs], usable)
    records, cnt = _miss_rows(B, ptrs, [0] * len(ptrs), [dt.ptr], n_rows, usable, cap=max(1, len(inputs) * n_rows))
    assert cnt == [missing, missing] and len(ref) == missing
    assert len(records) == missing and all(r[0] == 2 for r in records) and {r[1:] for r in records} == ref
    return counts, missing


# ---- collision chains -----------------------------------------------------------------------------------------------------------------------
N_CHAIN, U_CHAIN = 2048, 2042


def _base_words(rng):
    w = rng.integers(0, 1 << 32, 8, dtype=np.uint64).astype(np.uint32)
    w[7] = 0x0123abcd
    return w


def _chain_case(L, aimed, seed):
    """(table, inputs, keys of the chains): L colliding keys per chain on scattered rows of a random table; inputs with chain keys,
    colliding keys that are NOT in the table (they walk the whole chain to an empty slot) and ordinary keys"""
    rng = np.random.default_rng(seed)
    cap = ER.table_cap(U_CHAIN)
    if aimed == "wrap":                                        # the chain starts at the last slot and continues at slot 0
        bases = [ER.aim(_base_words(rng), cap, cap - 1)]
    elif aimed == "adjacent":                                  # two chains one slot apart: the first runs through the second
        bases = [ER.aim(_base_words(rng), cap, 1000), ER.aim(_base_words(rng), cap, 1001)]
    else:
        bases = [_base_words(rng)]
    chains = [ER.colliding_keys(L, b) for b in bases]
    for j, ch in enumerate(chains):                            # the aim, where there is one (not an expected value)
        assert len(set(ER.slot(ch, cap).tolist())) == 1
        if aimed != "free":
            assert int(ER.slot(ch, cap)[0]) == {"wrap": cap - 1, "adjacent": 1000 + j}[aimed]
    keys = np.stack(chains, axis=1).reshape(-1, 4)             # interleaved: a0 b0 a1 b1 ...
    absent = np.concatenate([ER.colliding_keys(64, b, first=100000) for b in bases])
    table = rand_fr(rng, N_CHAIN)
    rows = np.sort(rng.permutation(U_CHAIN)[:len(keys)])
    table[rows] = keys
    pick = lambda pool, n: pool[rng.integers(0, len(pool), n)]
    in0 = pick(keys, N_CHAIN)
    in1 = np.concatenate([pick(absent, 700), pick(keys, 700), pick(table[:U_CHAIN], N_CHAIN - 1400)])[rng.permutation(N_CHAIN)]
    in2 = pick(table[:U_CHAIN], N_CHAIN)
    in2[rng.integers(0, U_CHAIN, 9)] = rand_fr(rng, 9)
    for x in (in0, in1, in2):
        x[U_CHAIN:] = absent[:N_CHAIN - U_CHAIN]               # past `usable`: must not be counted
    return table, [in0, in1, in2], keys


@pytest.mark.parametrize("aimed", ["free", "wrap", "adjacent"])
@pytest.mark.parametrize("L", [2, 65, 600])
def test_collision_chains(B, L, aimed):
    table, inputs, keys = _chain_case(L, aimed, 1000 + L)
    counts, missing = _check_lookup(B, table, inputs, N_CHAIN, U_CHAIN)
    assert missing > 600 and counts.sum() + missing == 3 * U_CHAIN


def test_first_row_wins_under_a_race(B):
    """every key of a 65-key chain on three table rows, no two adjacent and the three in different workgroups: the counts land on the
    lowest of the three and nowhere else (atomicCAS to claim the slot, atomicMin among equal keys, other keys probing past)"""
    rng = np.random.default_rng(41)
    L = 65
    keys = ER.colliding_keys(L, _base_words(rng))
    table = rand_fr(rng, N_CHAIN)
    groups = [3 * rng.permutation(L), 701 + 3 * rng.permutation(L), 1500 + 3 * rng.permutation(L)]      # workgroups 0, 2-3, 5-6
    for g in groups:
        table[g] = keys
    table[1800:1900] = table[300:400]                          # ordinary keys twice as well, workgroups 1 and 7
    inputs = [keys[rng.integers(0, L, N_CHAIN)], table[rng.integers(0, U_CHAIN, N_CHAIN)]]
    counts, missing = _check_lookup(B, table, inputs, N_CHAIN, U_CHAIN)
    assert missing == 0 and (counts[groups[0]] > 0).all()
    assert not counts[groups[1]].any() and not counts[groups[2]].any() and not counts[1800:1900].any()


# ---- runs of equal table rows -----------------------------------------------------------------------------------------------------------
N_RUN, U_RUN = 1024, 1018
RUNS = {"rows 60-69": (60, 70), "rows 250-259": (250, 260), "from row 64": (64, 71), "up to row 63": (57, 64), "one wave": (128, 192),
        "whole table": (0, N_RUN)}


@pytest.mark.parametrize("name", list(RUNS))
def test_runs_of_equal_rows(B, name):
    """a run across a wave boundary, across a workgroup boundary, starting at lane 0, ending at lane 63, filling a wave, and a table
    that is one value: the run's count is on its first row"""
    a, b = RUNS[name]
    rng = np.random.default_rng(a * 1024 + b)
    table = rand_fr(rng, N_RUN)
    table[a:b] = table[a]
    rows = rng.integers(0, U_RUN, N_RUN)
    rows[::5] = rng.integers(a, min(b, U_RUN), len(rows[::5]))                  # the run, by any of its rows
    rows[1::50] = max(a - 1, 0)
    rows[2::50] = min(b, U_RUN - 1)
    inputs = [table[rows], table[rows[::-1]]]
    inputs[1][7::100] = rand_fr(rng, len(inputs[1][7::100]))
    counts, missing = _check_lookup(B, table, inputs, N_RUN, U_RUN)
    assert missing == len(inputs[1][7:U_RUN:100]) and counts[a] > N_RUN // 5 and not counts[a + 1:b].any()


@pytest.mark.parametrize("zero_is_usable", [True, False])
def test_zero_rows_at_the_usable_edge(B, zero_is_usable):
    """the table is the zero element from row usable - 3 (or from row usable) to its end, where the build pass's lanes past `usable`
    carry a zero key of their own: inputs that hold zero count on row usable - 3 (or are missing)"""
    rng = np.random.default_rng(17 + zero_is_usable)
    table = rand_fr(rng, N_RUN)
    first_zero = U_RUN - 3 if zero_is_usable else U_RUN
    table[first_zero:] = 0
    inputs = [table[rng.integers(0, U_RUN, N_RUN)] for _ in range(2)]
    inputs[0][3::7] = 0
    inputs[1][U_RUN - 1] = 0
    n_zero = sum(int((x[:U_RUN] == 0).all(axis=1).sum()) for x in inputs)
    assert n_zero > len(inputs[0][3:U_RUN:7])
    counts, missing = _check_lookup(B, table, inputs, N_RUN, U_RUN)
    if zero_is_usable:
        assert missing == 0 and counts[first_zero] == n_zero and not counts[first_zero + 1:].any()
    else:
        assert missing == n_zero and not counts[U_RUN:].any()


# ---- distinct targets per wave of the count pass ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("usable", [9 * 64 + 1, 9 * 64 + 63])
def test_targets_per_wave(B, usable):
    """waves 0-5 of the input hold exactly 1, 2, 3, 4, 5 and 64 distinct table values (three leader rounds, then one by one); wave 6 has
    its even lanes missing (lane 0 leads with `missing`); wave 7 has lane 63 missing behind 3 distinct hits (missing goes one by one),
    wave 8 behind 1 (missing leads the second round); wave 9 is ragged: 1 or 63 live lanes, one of them missing"""
    n_rows = 1024
    rng = np.random.default_rng(usable)
    table = rand_fr(rng, n_rows)
    absent = rand_fr(rng, 128)

    def wave(d):
        vals = table[rng.choice(500, d, replace=False)]
        return vals[rng.permutation(np.arange(64) % d)]
    col = np.concatenate([wave(d) for d in (1, 2, 3, 4, 5, 64)] + [wave(2), wave(3), wave(1), wave(2)] + [absent[:64]] * 6)
    col[6 * 64:7 * 64:2] = absent[64:96]
    col[7 * 64 + 63] = absent[100]
    col[8 * 64 + 63] = absent[101]
    col[9 * 64 + 5] = absent[102]
    distinct = [len({x.tobytes() for x in col[64 * w:64 * w + 64]}) for w in range(10)]
    assert distinct == [1, 2, 3, 4, 5, 64, 2 + 32, 3 + 1, 1 + 1, 2 + 1]
    inputs = [col, table[rng.integers(0, 500, n_rows)]]
    counts, missing = _check_lookup(B, table, inputs, n_rows, usable)
    assert missing == 32 + 2 + (usable > 9 * 64 + 5) and not counts[500:].any()


# ---- the `usable` edge ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("usable", [0, 1, 2, 511, 512])
def test_usable_edges(B, usable):
    """table rows at or past `usable` are not found, input rows at or past it are not counted, the output past it is zero.  usable = 0
    with inputs present gives an all-zero column and missing == 0: that is what lookup_multiplicity_batch does (no pass is launched).
    mv_lookup::prover::prepare is not in the reference project's tree (it belongs to its halo2 dependency), so this follows the
    kernel: with no usable row there is no input row to count or to miss."""
    n_rows = 512
    rng = np.random.default_rng(300 + usable)
    table = rand_fr(rng, n_rows)
    only_past = rand_fr(rng, 4)
    table[usable:usable + 4] = only_past[:len(table[usable:usable + 4])]       # values that occur only at or past `usable`
    inputs = [table[rng.integers(0, max(1, usable), n_rows)] for _ in range(2)]
    inputs[0][0], inputs[1][0] = only_past[0], table[0]
    if usable > 1:
        inputs[1][usable - 1] = only_past[1]
    counts, missing = _check_lookup(B, table, inputs, n_rows, usable)
    if usable == 0:
        assert missing == 0 and not counts.any()
    else:
        assert missing == 1 + (usable > 1) and counts.sum() + missing == 2 * usable
    changed = [x.copy() for x in inputs]                       # inputs that differ only at or past `usable` change nothing
    for x in changed:
        x[usable:] = rand_fr(rng, n_rows - usable)
    assert _check_lookup(B, table, changed, n_rows, usable)[1] == missing
    dt, d0, d1 = _dev(B, [table])[0], _dev(B, inputs), _dev(B, changed)
    m0, _ = B.lookup_multiplicity([d.ptr for d in d0], dt.ptr, n_rows, usable)
    m1, _ = B.lookup_multiplicity([d.ptr for d in d1], dt.ptr, n_rows, usable)
    assert (_column(m0, n_rows) == _column(m1, n_rows)).all() and not _column(m0, n_rows)[usable:].any()


# ---- the accumulated missing counter, and a batch with interleaved inputs --------------------------------------------------------------------
def test_accumulated_missing_counter(B):
    """ezkl_hip_lookup_multiplicity_acc_dev twice on one device counter preset to 7, queued without synchronising (asynchronous library
    stream, as the native prover calls it) and read once: 7 + a + b, and each call's column is the plain form's"""
    from ezkl_amd import lib as L
    t_a, in_a, _ = _chain_case(65, "wrap", 77)
    rng = np.random.default_rng(78)
    n_b, u_b = 1024, 1000
    t_b = rand_fr(rng, n_b)
    in_b = [t_b[rng.integers(0, u_b, n_b)] for _ in range(2)]
    in_b[0][::9] = rand_fr(rng, len(in_b[0][::9]))
    sets = [(t_a, in_a, N_CHAIN, U_CHAIN), (t_b, in_b, n_b, u_b)]
    refs = [ER.multiplicity(*s) for s in sets]
    assert refs[0][1] > 0 and refs[1][1] > 0 and refs[0][1] != refs[1][1]
    counter = B.DeviceBuffer.from_numpy(np.array([7], np.uint32))
    dev = [(_dev(B, [t])[0], _dev(B, ins), B.DeviceBuffer(n * 32)) for t, ins, n, _ in sets]
    keep = []
    prev = B.set_async(True)
    try:
        for (dt, di, out), (_, _, n, u) in zip(dev, sets):
            arr = (C.c_void_p * len(di))(*[d.ptr for d in di])
            keep.append(arr)
            L.check(L.load().ezkl_hip_lookup_multiplicity_acc_dev(arr, C.c_uint32(len(di)), C.c_void_p(dt.ptr), C.c_uint32(n), C.c_uint32(u),
                                                                  C.c_void_p(out.ptr), C.c_void_p(counter.ptr), C.c_void_p(None)),
                    "ezkl_hip_lookup_multiplicity_acc_dev")
        total = int(counter.to_numpy(np.uint32)[0])             # the one read, behind both calls on the library stream
    finally:
        B.set_async(prev)
    assert total == 7 + refs[0][1] + refs[1][1]
    for (dt, di, out), (_, _, n, u), (counts, missing) in zip(dev, sets, refs):
        plain, miss = B.lookup_multiplicity([d.ptr for d in di], dt.ptr, n, u)
        assert miss == missing
        assert (_column(out, n) == ER.counts_to_fr(counts)).all() and (_column(out, n) == _column(plain, n)).all()


def test_batch_with_interleaved_inputs(B):
    """one batch call over arguments with 0, 1 and 4 inputs whose items are NOT sorted by argument (which = 2 2 1 2 2), the 4-input
    argument on the chain table: every column equals the one-argument call and the reference; the miss report numbers each input
    by its position among its own argument's inputs"""
    from ezkl_amd import lib as L
    t2, in2, keys = _chain_case(65, "adjacent", 91)
    rng = np.random.default_rng(92)
    in2.append(keys[rng.integers(0, len(keys), N_CHAIN)])
    t0, t1 = rand_fr(rng, N_CHAIN), rand_fr(rng, N_CHAIN)
    in1 = [t1[rng.integers(0, U_CHAIN, N_CHAIN)]]
    in1[0][11::100] = rand_fr(rng, len(in1[0][11::100]))
    tables, inputs = [t0, t1, t2], [[], in1, in2]
    refs = [ER.multiplicity(t, ins, N_CHAIN, U_CHAIN) for t, ins in zip(tables, inputs)]
    dt, di = _dev(B, tables), [_dev(B, ins) for ins in inputs]
    which = [2, 2, 1, 2, 2]
    flat = [di[2][0].ptr, di[2][1].ptr, di[1][0].ptr, di[2][2].ptr, di[2][3].ptr]
    outs = [B.DeviceBuffer(N_CHAIN * 32) for _ in range(3)]
    miss = B.DeviceBuffer.from_numpy(np.zeros(1, np.uint32))
    a_in, a_which = (C.c_void_p * 5)(*flat), (C.c_uint32 * 5)(*which)
    a_tab, a_out = (C.c_void_p * 3)(*[d.ptr for d in dt]), (C.c_void_p * 3)(*[o.ptr for o in outs])
    L.check(L.load().ezkl_hip_lookup_multiplicity_batch_dev(a_in, a_which, C.c_uint32(5), a_tab, C.c_uint32(3), C.c_uint32(N_CHAIN), C.c_uint32(U_CHAIN),
                                                            a_out, C.c_void_p(miss.ptr), C.c_void_p(None)), "ezkl_hip_lookup_multiplicity_batch_dev")
    assert int(miss.to_numpy(np.uint32)[0]) == sum(m for _, m in refs) and refs[1][1] > 0 and refs[2][1] > 0
    for l in range(3):
        one, miss_one = B.lookup_multiplicity([d.ptr for d in di[l]], dt[l].ptr, N_CHAIN, U_CHAIN)
        assert miss_one == refs[l][1]
        assert (_column(outs[l], N_CHAIN) == _column(one, N_CHAIN)).all() and (_column(one, N_CHAIN) == ER.counts_to_fr(refs[l][0])).all()
    assert not _column(outs[0], N_CHAIN).any()
    records, cnt = _miss_rows(B, flat, which, [d.ptr for d in dt], N_CHAIN, U_CHAIN, cap=5 * N_CHAIN)
    assert cnt == [sum(m for _, m in refs)] + [m for _, m in refs]
    assert len(records) == cnt[0] and {r[1:] for r in records} == ER.miss_records(tables, inputs, U_CHAIN)


# ---- the record cap of the two reports --------------------------------------------------------------------------------------------------
CAPS = [0, 1, 39, 40, 41, 100, 101]


@pytest.fixture(scope="module")
def hundred_misses(B):
    """two arguments, 100 missing input rows: 40 in one wave of argument 0's first input, 1 alone in its second, 59 spread over
    argument 1's only input; absent values past `usable` as well"""
    rng = np.random.default_rng(55)
    tables = [rand_fr(rng, N_RUN) for _ in range(2)]
    inputs = [[tables[0][rng.integers(0, U_RUN, N_RUN)] for _ in range(2)], [tables[1][rng.integers(0, U_RUN, N_RUN)]]]
    inputs[0][0][192 + rng.permutation(64)[:40]] = rand_fr(rng, 40)
    inputs[0][1][700] = rand_fr(rng, 1)[0]
    inputs[1][0][5:5 + 17 * 59:17] = rand_fr(rng, 59)
    for x in inputs[0] + inputs[1]:
        x[U_RUN:] = rand_fr(rng, N_RUN - U_RUN)
    ref = ER.miss_records(tables, inputs, U_RUN)
    assert len(ref) == 100 and sum(r[0] == 0 for r in ref) == 41
    return _dev(B, tables), [_dev(B, ins) for ins in inputs], ref


@pytest.mark.parametrize("cap", CAPS)
def test_miss_report_cap(B, hundred_misses, cap):
    dt, di, ref = hundred_misses
    flat = [d.ptr for ins in di for d in ins]
    records, cnt = _miss_rows(B, flat, [0, 0, 1], [d.ptr for d in dt], N_RUN, U_RUN, cap)
    assert cnt == [100, 41, 59]
    assert len(records) == min(cap, 100) == len(set(records)) and all(r[0] == 2 for r in records)
    assert {r[1:] for r in records} <= ref
    if cap >= 100:
        assert {r[1:] for r in records} == ref


@pytest.fixture(scope="module")
def hundred_bad_cells(B):
    """m = 3 columns of 2^10 rows whose successor map has 100 bad cells: 40 in one wave, the first cell, the last cell of the last
    column, a successor of exactly m n (the first cell outside), one of 0xffffffff, and 56 spread; good cells: fixed points and 20
    cycles of 8 equal cells"""
    rng = np.random.default_rng(56)
    log_n, m = 10, 3
    n, cells = 1 << log_n, 3 << 10
    flat = rand_fr(rng, cells)
    nxt = np.arange(cells, dtype=np.uint32)                    # every cell a loop on itself, whose value is fine
    order = rng.permutation(np.arange(1, cells - 1))
    order = order[(order < 640) | (order >= 704)]
    for cyc in order[:160].reshape(20, 8):
        nxt[cyc] = np.roll(cyc, -1)
        flat[cyc] = flat[cyc[0]]
    free = order[160:]
    bad = np.concatenate([[0, cells - 1], 640 + rng.permutation(64)[:40], free[:58]])
    nxt[bad] = free[100:200]                                   # a successor with another value
    nxt[free[56]], nxt[free[57]] = cells, 0xffffffff
    cols = flat.reshape(m, n, 4)
    ref = ER.copy_bad(cols, nxt, log_n)
    assert len(ref) == 100 and {(0, 0), (m - 1, n - 1)} <= ref
    return _dev(B, list(cols)), B.DeviceBuffer.from_numpy(nxt), log_n, ref


@pytest.mark.parametrize("cap", CAPS)
def test_copy_report_cap(B, hundred_bad_cells, cap):
    dc, dn, log_n, ref = hundred_bad_cells
    records, cnt = _copy_check(B, [d.ptr for d in dc], dn.ptr, log_n, cap)
    assert cnt == [100]
    assert len(records) == min(cap, 100) == len(set(records)) and all(r[0] == 3 and r[2] == 0 for r in records)
    assert {(r[1], r[3]) for r in records} <= ref
    if cap >= 100:
        assert {(r[1], r[3]) for r in records} == ref


def test_report_bindings_agree_with_the_guarded_calls(B, hundred_misses, hundred_bad_cells):
    """backend.lookup_missing_rows / copy_check (their own record buffers) on the same inputs"""
    dt, di, ref = hundred_misses
    for cap in (39, 128):
        records, cnt = B.lookup_missing_rows([[d.ptr for d in ins] for ins in di], [d.ptr for d in dt], N_RUN, U_RUN, cap=cap)
        assert cnt == [100, 41, 59] and len(records) == min(cap, 100) and {r[1:] for r in records} <= ref
    assert {r[1:] for r in records} == ref
    dc, dn, log_n, bad = hundred_bad_cells
    for cap in (39, 128):
        records, cnt = B.copy_check([d.ptr for d in dc], dn.ptr, log_n, cap=cap)
        assert cnt == [100] and len(records) == min(cap, 100) and {(r[1], r[3]) for r in records} <= bad
    assert {(r[1], r[3]) for r in records} == bad


# ---- past the first pass of the grid ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid_pass(hip):
    """elements one pass of a streaming kernel's grid covers: stream_grid caps it at 8 workgroups of 256 lanes per compute unit"""
    import subprocess
    import sys
    # torch's HIP runtime does not find the device once the library's runtime holds it in this process (tests/test_rowshard.py
    # starts torch first for the same reason), so one fresh child asks torch
    out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                         check=True, capture_output=True, text=True, timeout=120).stdout
    return 8 * int(out.split()[-1]) * 256


def test_vec_ops_past_the_grid(B, grid_pass):
    """vec_op add / sub / mul, vec_scale and vec_fill on G + 257 elements: a second pass with a ragged tail, every element compared"""
    n = grid_pass + 257
    rng = np.random.default_rng(61)
    a, b, s = rand_fr(rng, n), rand_fr(rng, n), rand_fr(rng, 1)[0]
    da, db = _dev(B, [a, b])
    out = B.DeviceBuffer.from_numpy(np.full((n + 1, 4), GUARD, np.uint64))
    for op in ("add", "sub", "mul"):
        B.vec_op(op, da.ptr, db.ptr, out.ptr, n)
        got = _column(out, n + 1)
        assert (got[:n] == ob.vec_op(op, a, b)).all() and (got[n] == GUARD).all(), op
    B.vec_scale(da.ptr, s, out.ptr, n)
    got = _column(out, n + 1)
    assert (got[:n] == ob.vec_scale(a, s)).all() and (got[n] == GUARD).all()
    B.vec_fill(out.ptr, s, n)
    got = _column(out, n + 1)
    assert (got[:n] == s).all() and (got[n] == GUARD).all()
    assert (_column(da, n) == a).all() and (_column(db, n) == b).all()


def test_permutation_sigma_past_the_grid(B, grid_pass):
    """one sigma column of 2^k > G rows (a whole second pass; the row count is a power of two, so there is no ragged tail): successors
    in both of m = 2 columns and three outside them in the second pass, every row against a gather over the omega column times
    delta^c through the oracle"""
    from oracle import pyref as pr
    k = grid_pass.bit_length()
    n, m = 1 << k, 2
    assert n > grid_pass >= n // 2
    rng = np.random.default_rng(62)
    wcol = ob.prefix_scan(np.tile(ob.omega(k), (n, 1)), "mul", exclusive=True)                       # omega^r, r = 0 .. n - 1
    assert (wcol[0] == fe_from_int(1)).all() and (wcol[1] == ob.omega(k)).all() and (ob.fr_mul(wcol[n - 1], ob.omega(k)) == fe_from_int(1)).all()
    dpow = np.stack([fe_from_int(pow(pr.DELTA, c, R)) for c in range(m)])
    nxt = rng.integers(0, m * n, n, dtype=np.uint32)
    nxt[::3] = np.arange(n, dtype=np.uint32)[::3]                                                     # fixed points of column 0
    outside = [grid_pass, grid_pass + 1000, n - 1]
    nxt[outside] = [m * n, m * n + 12345, 0xffffffff]
    d_w, d_d, d_n = _dev(B, [wcol, dpow, nxt])
    out = B.DeviceBuffer(32 * n)
    B.permutation_sigma_dev(d_n.ptr, d_w.ptr, d_d.ptr, m, k, out.ptr)
    got = _column(out, n)
    inside = nxt < m * n
    want = np.zeros((n, 4), np.uint64)
    for c in range(m):
        sel = inside & (nxt >> k == c)
        assert sel[grid_pass:].any()
        want[sel] = ob.vec_scale(wcol[nxt[sel] & (n - 1)], dpow[c])
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:8]
    assert not got[outside].any()


def test_copy_check_past_the_grid(B, grid_pass):
    """m = 3 columns at the smallest height with more than G cells: 50 bad cells, 25 of them in the second pass of the whole-wave
    loop, one the last cell of all; exact records and total"""
    m, log_n = 3, 0
    while (m << log_n) <= grid_pass:
        log_n += 1
    n, cells = 1 << log_n, m << log_n
    assert cells > grid_pass
    rng = np.random.default_rng(63)
    flat = rand_fr(rng, cells)
    nxt = np.arange(cells, dtype=np.uint32)
    cyc = rng.permutation(cells - 1)[:40000].reshape(-1, 8)    # 5000 cycles of 8 equal cells, across both passes
    for j in range(8):
        nxt[cyc[:, j]] = cyc[:, (j + 1) % 8]
        flat[cyc[:, j]] = flat[cyc[:, 0]]
    fixed = np.nonzero(nxt == np.arange(cells))[0]              # the bad cells: fixed points sent to a neighbour with another value
    lo, hi = fixed[fixed < grid_pass], fixed[(fixed >= grid_pass) & (fixed < cells - 1)]
    bad = np.concatenate([rng.choice(lo, 25, replace=False), rng.choice(hi, 24, replace=False), [cells - 1]])
    nxt[bad] = (bad + 1) % cells
    cols = flat.reshape(m, n, 4)
    ref = ER.copy_bad(cols, nxt, log_n)
    assert len(ref) == 50
    dc, dn = _dev(B, list(cols)), B.DeviceBuffer.from_numpy(nxt)
    records, cnt = _copy_check(B, [d.ptr for d in dc], dn.ptr, log_n, cap=64)
    assert cnt == [50] and len(records) == 50 and {(r[1], r[3]) for r in records} == ref
    assert (m - 1, n - 1) in ref and sum((c << log_n) + r >= grid_pass for c, r in ref) == 25
