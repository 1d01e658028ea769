"""The lookup-statistics kernel (csrc/witness.hip wit_lookup_stats_kernel, ezkl_hip_witness_lookup_stats_dev) against its specification
`witness_plan.lookup_stats_host` and against the closed form min(0, sources), max(0, sources) of the planted values, on synthetic plans
built as tests/witness_synth.py builds them -- one nonlinearity record of every count around a wave, a workgroup and the grid's first
stride; three such records among other kinds; none -- and on the recorded conv and softmax plans after a real replay."""
import numpy as np
import pytest

import witness_synth as S

pytestmark = pytest.mark.gpu
LO, HI = -5000, 5000                                # the synthetic table's range: f(x) = x // 4 over it
COUNTS = [1, 63, 64, 65, 257, 4097]                 # 4097: past one workgroup of 256 lanes, a second trip of no lane


def _table(b):
    return b.table(LO, 2501, [x // 4 for x in range(LO, HI + 1)])


def _single(count):
    """INPUT -> `count` cells, one TABLE record over them; the inputs are the sources, in order"""
    b = S.Builder(13, 2)
    src = b.input(b.fresh(count, corner=True), [0] * count)
    b.lookup(b.fresh(count, corner=True), src, _table(b))
    return b.plan()


def _check(B, WP, dev, cols, plan, x, want):
    dev.run(x, columns=cols)
    assert dev.last["failed"] == 0
    got = dev.lookup_stats(cols)
    assert got == want, "device %s, closed form %s" % (got, want)
    assert got == WP.lookup_stats_host(plan, WP.run_plan_host(plan, x)[0])
    assert dev.last_stats_ms is not None and dev.last_stats_ms >= 0 and B.last_kernel_ms("witness_lookup_stats") >= 0


@pytest.mark.parametrize("count", COUNTS)
def test_one_record_extremum_in_the_first_the_last_and_a_mid_wave_element(hip, count):
    """every call on the same plan and the same columns after other inputs: the result words are set again by each call"""
    from ezkl_amd import backend as B, witness_plan as WP
    plan = _single(count)
    dev = B.WitnessPlan(plan.to_bytes())
    cols = dev.alloc_columns()
    rng = np.random.default_rng(count)
    try:
        assert dev.n_lookup_records == 1
        for at in sorted({0, count - 1, min(37, count // 2), count // 2}):
            for sign in (1, -1):                                     # the greatest alone at `at`, then the least
                x = rng.integers(-900, 901, count).tolist()
                x[at] = sign * 4321
                want = (min(0, *x), max(0, *x))
                assert want[0 if sign < 0 else 1] == sign * 4321
                _check(B, WP, dev, cols, plan, x, want)
        pos = rng.integers(1, 900, count).tolist()                   # all sources positive: the minimum stays 0
        _check(B, WP, dev, cols, plan, pos, (0, max(pos)))
        neg = [-v for v in pos]                                      # all negative: the maximum stays 0
        _check(B, WP, dev, cols, plan, neg, (min(neg), 0))
        _check(B, WP, dev, cols, plan, [0] * count, (0, 0))
        ends = [(LO, HI)[i % 2] for i in range(count)]               # the table bounds themselves
        _check(B, WP, dev, cols, plan, ends, (LO, HI if count > 1 else 0))
    finally:
        for c in cols:
            c.free()
        dev.free()


GRID_LANES = 256 * 256                              # csrc/witness.hip: STATS_MAX_BLOCKS workgroups of STATS_THREADS lanes


def test_elements_past_the_grid_are_reached_by_the_stride(hip):
    """one record of GRID_LANES + 64 elements: the first GRID_LANES read 64 small sources over and over, the last 64 -- the second trip of
    the first wave -- alone read the cell that holds the extremum"""
    from ezkl_amd import backend as B, witness_plan as WP
    count = GRID_LANES + 64
    b = S.Builder(16, 3)
    src = b.input(b.fresh(65), [0] * 65)
    b.lookup(b.fresh(count), src.take([i % 64 if i < GRID_LANES else 64 for i in range(count)]), _table(b))
    plan = b.plan()
    dev = B.WitnessPlan(plan.to_bytes())
    cols = dev.alloc_columns()
    try:
        for tail in (4777, -4888):
            x = [(-1) ** i * (i + 1) for i in range(64)] + [tail]
            dev.run(x, columns=cols)
            assert dev.lookup_stats(cols) == (min(-64, tail), max(63, tail))
    finally:
        for c in cols:
            c.free()
        dev.free()


def _mixed():
    """three TABLE records over two tables among INPUT, COPY, ADD and TBLIDX records; the input with the greatest magnitude feeds an ADD only"""
    b = S.Builder(10, 4)
    vals = [7, -3, 1200, -2500, 40, -41, 3, 2999, -4999, 12, 1 << 40, -(1 << 41)] + list(range(-60, 60))
    src = b.input(b.fresh(len(vals), corner=True), vals)
    t0, t1 = _table(b), b.table(-64, 32, [x * x for x in range(-64, 64)])
    b.lookup(b.fresh(5), src.take(range(0, 5)), t0)                  # 7 .. 40: least -2500, greatest 1200
    moved = b.copy(b.fresh(4), src.take(range(5, 9)))                # -41, 3, 2999, -4999
    b.lookup_index(b.fresh(4), moved, t0)
    b.lookup(b.fresh(4, corner=True), moved, t0)                     # least -4999, greatest 2999
    b.add(b.fresh(2), src.take([10, 11]), src.take([11, 10]))        # 2^40 - 2^41: no lookup reads it
    b.lookup(b.fresh(120), src.take(range(12, 132)), t1)             # -60 .. 59
    return b.plan(), b.x, (-4999, 2999)


def test_three_records_among_other_kinds_and_a_plan_without_lookups(hip):
    from ezkl_amd import backend as B, witness_plan as WP
    plan, x, want = _mixed()
    kinds = plan.records[:, 0].tolist()
    assert kinds.count(WP.TABLE) == 3 and {WP.INPUT, WP.COPY, WP.ADD, WP.TBLIDX} <= set(kinds)
    dev = B.WitnessPlan(plan.to_bytes())
    cols = dev.alloc_columns()
    try:
        assert dev.n_lookup_records == 3
        _check(B, WP, dev, cols, plan, x, want)
    finally:
        for c in cols:
            c.free()
        dev.free()
    case = S.elementwise_case(65, "permuted", 1)                     # no TABLE record: (0, 0), nothing launched
    dev = B.WitnessPlan(case.plan.to_bytes())
    cols = dev.alloc_columns()
    try:
        dev.run(case.x, columns=cols)
        assert dev.n_lookup_records == 0 and dev.lookup_stats(cols) == (0, 0) and dev.last_stats_ms is None
        assert WP.lookup_stats_host(case.plan, case.columns()) == (0, 0)
    finally:
        for c in cols:
            c.free()
        dev.free()


def test_a_source_beyond_62_bits_is_an_error_status_not_an_extremum(hip):
    """columns no passing replay leaves: a lookup source holding 2^62 (and one holding -(2^62)), uploaded from the host"""
    from ezkl_amd import backend as B, ezkl_layout as EL, witness_plan as WP
    plan = _single(65)
    dev = B.WitnessPlan(plan.to_bytes())
    cols = []
    try:
        host, _ = WP.run_plan_host(plan, list(range(-32, 33)))
        assert WP.lookup_stats_host(plan, host) == (-32, 32)
        src = plan.pool[plan.records[1, 5]:plan.records[1, 5] + 65].tolist()
        for cell, v in ((src[3], 1 << 62), (src[64], -(1 << 62))):
            host[cell >> plan.k][cell & ((1 << plan.k) - 1)] = v % S.R
        with pytest.raises(ValueError, match=WP.STATS_ERROR):
            WP.lookup_stats_host(plan, host)
        cols = [B.DeviceBuffer.from_numpy(EL.ints_to_mont(c)) for c in host]
        with pytest.raises(B.WitnessError, match="2 lookup inputs beyond 62 bits"):
            dev.lookup_stats(cols)
        host[src[3] >> plan.k][src[3] & ((1 << plan.k) - 1)] = (1 << 62) - 1      # the greatest magnitude a lane holds
        host[src[64] >> plan.k][src[64] & ((1 << plan.k) - 1)] = (-(1 << 62) + 1) % S.R
        for c in cols:
            c.free()
        cols = [B.DeviceBuffer.from_numpy(EL.ints_to_mont(c)) for c in host]
        assert dev.lookup_stats(cols) == (-(1 << 62) + 1, (1 << 62) - 1) == WP.lookup_stats_host(plan, host)
    finally:
        for c in cols:
            c.free()
        dev.free()


def _conv_k10():
    from ezkl_amd import ezkl_layout as EL
    c = EL.ConvMnistCircuit(logrows=10, image=8, kernel=3, out_channels=2, stride=2, classes=3, lookup_range=(-700, 700), denom=4, decomp_base=32, decomp_legs=2)
    return c, np.random.default_rng(1).integers(0, 4, 64).tolist()


def _softmax():
    from ezkl_amd import ezkl_layout as EL
    return EL.NormCircuit(9, 2, 3000, 2, 4), [1, 5, -3, 7, 0, 0, 2, 9]


@pytest.mark.parametrize("make", [_conv_k10, _softmax], ids=["conv_k10", "norm_softmax"])
def test_recorded_plans_after_a_real_replay_give_the_layouts_statistics(hip, make):
    from ezkl_amd import backend as B, witness_plan as WP
    circuit, x = make()
    reg = circuit.synthesize(x)
    want = (reg.min_lookup_inputs, reg.max_lookup_inputs)
    assert want != (0, 0)
    plan = WP.record_plan(circuit)
    dev = B.WitnessPlan(plan.to_bytes())
    cols, outs = dev.run(x)
    try:
        assert outs == circuit.outputs
        assert dev.lookup_stats(cols) == want == WP.lookup_stats_host(plan, WP.run_plan_host(plan, x)[0])
    finally:
        for c in cols:
            c.free()
        dev.free()
