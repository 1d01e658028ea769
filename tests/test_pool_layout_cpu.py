"""`BaseRegion.argmax` / `argmin` / `argmax_axes` / `argmin_axes`, `select`, `max_pool` and `sumpool` (ezkl_layout.py, after layouts.rs:5225-5293,
:2781-2905, :1363-1396, :4008-4087 and :3907-3980) under the mock prover: the doc examples of the reference, segments of one, two and seven
elements, all-equal values, padding and strides other than one; the engine's claim is accepted in both modes, a claim moved to another
position of the same extremum or to another value is reported; PoolClassifierCircuit proves its integer forward pass with both poolings."""
import numpy as np
import pytest


class OpCircuit:
    """one op on a private vector assigned on the first input VarTensor: instance = what `op(reg, cells)` returns"""

    def __init__(self, n_inputs, n_outputs, op, sorts=0, sort_rows=0, selects=0, select_rows=0, k=9, w=2, capacity=4000, decomp=(16, 2)):
        from ezkl_amd import ezkl_circuit as EC
        self.k, self.w, self.n_inputs, self.op, self.decomp = k, w, n_inputs, op, decomp
        self.settings = EC.GraphSettings(k, w, capacity, total_const_size=8, required_range_checks=[(-1, 1), (0, decomp[0] - 1), (0, 1)],
                                         model_instance_shapes=[[1, n_outputs]], total_shuffle_col_size=sort_rows, num_shuffles=sorts,
                                         total_dynamic_col_size=select_rows, num_dynamic_lookups=selects)
        self.gc = EC.GraphConfig(self.settings)

    def layout(self, reg, inputs, param):
        reg.decomp = self.decomp
        vals = reg.assign(reg.inputs[0], inputs)
        reg.increment(len(vals))
        outs = self.op(reg, vals)
        reg.constrain_instance(outs, self.gc.instance)
        return outs

    def plan_identity(self):
        return b"one op"

    def synthesize(self, x, witness=True, region=None):
        from ezkl_amd import ezkl_layout as EL
        reg = (region or EL.BaseRegion)(self.gc, witness)
        outs = self.layout(reg, [EL.Val(int(v) % EL.R) for v in x], EL.Val)
        reg.finish(self.gc.const_cols)
        self.outputs = [v.v for v in outs]
        return reg


def arg_circuit(rows, length, mode):
    """`argmax_axes` / `argmin_axes` over `rows` rows of `length`"""
    op = lambda reg, vals: getattr(reg, "arg%s_axes" % mode)([vals[r * length:(r + 1) * length] for r in range(rows)])
    many = length > 1
    return OpCircuit(rows * length, rows, op, sorts=rows * many, sort_rows=rows * length * many, selects=rows, select_rows=rows * length)


def checked(c, x, key_x=None, region=None, **kw):
    """(mock prover failures, instance as signed integers): keys from `key_x` (the layout does not depend on the values), witness from x"""
    from ezkl_amd import ezkl_layout as EL
    from oracle import mock_prover as MP
    reg = c.synthesize(x, region=region) if region else c.synthesize(x)
    n = 1 << c.k
    adv = [list(reg.advice.get(col.index) or [0] * n) for col in c.gc.cs.advice]
    outputs = list(c.outputs)
    cs, fixed, copies, _ = EL.LayoutCircuit.keygen_inputs(c, x if key_x is None else key_x)       # (last: it rewrites the system in place)
    return MP.check(cs, adv, [list(f) for f in fixed], [outputs], list(copies), **kw), [EL.signed(v) for v in outputs]


def closed_form(seg, mode):
    return max(range(len(seg)), key=lambda j: (seg[j], -j)) if mode == "max" else min(range(len(seg)), key=lambda j: (seg[j], j))


def test_the_doc_example_of_argmax_axes_and_the_tie_goes_to_the_first_index():
    x = [2, 15, 2, 1, 1, 0]
    fails, inst = checked(arg_circuit(2, 3, "max"), x)
    assert fails == [] and inst == [1, 0]
    fails, inst = checked(arg_circuit(2, 3, "min"), x)
    assert fails == [] and inst == [0, 2]


@pytest.mark.parametrize("mode", ["max", "min"])
@pytest.mark.parametrize("length", [1, 2, 7])
def test_the_engines_claim_is_accepted(length, mode):
    rng = np.random.default_rng(length)
    rows = [rng.integers(-3, 4, length).tolist(), [5] * length, list(range(length)), list(range(length, 0, -1))]     # ties, all equal, the last, the first
    x = [v for row in rows for v in row]
    fails, inst = checked(arg_circuit(len(rows), length, mode), x, key_x=[0] * len(x))
    assert fails == []
    assert inst == [closed_form(row, mode) for row in rows]
    if length > 1:
        assert inst[1] == 0, "all equal: the first position"


def test_arg_extremum_is_the_smallest_position_and_asserts_its_range():
    from ezkl_amd import ezkl_layout as EL
    reg = EL.BaseRegion(arg_circuit(1, 7, "max").gc)
    vals = [EL.Val(v) for v in (5, -2, 7, 7, -9, -9, 0)]
    assert reg._arg_extremum(vals, "max") == 2 and reg._arg_extremum(vals, "min") == 4
    assert EL.ARGEXT_ERROR == "arg-extremum key beyond 62 bits"
    for bad in (1 << 62, -(1 << 62)):
        with pytest.raises(AssertionError, match=EL.ARGEXT_ERROR):
            reg._arg_extremum(vals + [EL.Val(bad)], "max")
    assert reg._arg_extremum([EL.Val((1 << 62) - 1), EL.Val(-(1 << 62) + 1)], "min") == 1


def _cheat(move):
    """a BaseRegion whose `_arg_extremum` answers move(honest claim)"""
    from ezkl_amd import ezkl_layout as EL

    class Cheat(EL.BaseRegion):
        def _arg_extremum(self, vals, mode):
            return move(EL.BaseRegion._arg_extremum(self, vals, mode))
    return Cheat


@pytest.mark.parametrize("mode", ["max", "min"])
def test_a_claim_at_another_position_of_the_same_extremum_is_reported(mode):
    """[4, 9, 1, 9, 1, 4, 0 / 10]: the extremum twice; the later of the two positions is the same VALUE -- `select` and the first equality
    hold -- and the claimed index is not the one the indexed sort puts at its end: the tie rule"""
    x = [4, 9, 1, 9, 1, 4, 5]
    honest, other = (1, 3) if mode == "max" else (2, 4)
    fails, inst = checked(arg_circuit(1, 7, mode), x)
    assert fails == [] and inst == [honest]
    fails, inst = checked(arg_circuit(1, 7, mode), x, region=_cheat(lambda j: other), max_failures=64)
    assert inst == [other] and fails and all(f.startswith("copy") for f in fails), fails[:3]


@pytest.mark.parametrize("mode", ["max", "min"])
def test_a_claim_at_another_value_is_reported(mode):
    x = [4, 9, 1, 9, 1, 4, 5]
    fails, inst = checked(arg_circuit(1, 7, mode), x, region=_cheat(lambda j: 6), max_failures=64)
    assert inst == [6] and fails and all(f.startswith("copy") for f in fails), fails[:3]


def test_a_claim_outside_the_segment_is_reported_by_the_lookup():
    """an index no table row has: the dynamic lookup of `select` fails (the engine itself refuses to lay it out: GATHER_ERROR)"""
    from ezkl_amd import ezkl_layout as EL
    c = arg_circuit(1, 7, "max")
    with pytest.raises(AssertionError, match=EL.GATHER_ERROR):
        c.synthesize([4, 9, 1, 9, 1, 4, 5], region=_cheat(lambda j: 7))


# ---- pooling ---------------------------------------------------------------------------------------------------------------------------
def pool_circuit(kind, channels, height, width, padding, stride, pool, normalized=False):
    H, W = (padding[0][0] + height + padding[0][1], padding[1][0] + width + padding[1][1])
    slides = ((H - pool[0]) // stride[0] + 1, (W - pool[1]) // stride[1] + 1)
    n_out = channels * slides[0] * slides[1]
    if kind == "max":
        op = lambda reg, vals: reg.max_pool(vals, channels, height, width, padding, stride, pool)
        return OpCircuit(channels * height * width, n_out, op, sorts=n_out, sort_rows=n_out * pool[0] * pool[1], k=10, capacity=8000, decomp=(16, 3)), slides
    op = lambda reg, vals: reg.sumpool(vals, channels, height, width, padding, stride, pool, normalized)
    return OpCircuit(channels * height * width, n_out, op, k=10, capacity=8000, decomp=(16, 3)), slides


def windows(x, channels, height, width, padding, stride, pool, slides):
    img = np.pad(np.asarray(x, np.int64).reshape(channels, height, width), ((0, 0), padding[0], padding[1]))
    return [img[c, i * stride[0]:i * stride[0] + pool[0], j * stride[1]:j * stride[1] + pool[1]]
            for c in range(channels) for i in range(slides[0]) for j in range(slides[1])]


def test_the_doc_example_of_max_pool():
    """layouts.rs:3999-4005"""
    c, _ = pool_circuit("max", 1, 3, 3, ((0, 0), (0, 0)), (1, 1), (2, 2))
    fails, inst = checked(c, [5, 2, 3, 0, 4, -1, 3, 1, 6])
    assert fails == [] and inst == [5, 4, 4, 6]


GEOMETRIES = [(1, 3, 3, ((0, 0), (0, 0)), (1, 1), (2, 2)), (2, 4, 5, ((1, 1), (1, 0)), (2, 2), (2, 2)), (1, 5, 4, ((0, 1), (2, 0)), (2, 1), (3, 2)),
              (1, 2, 2, ((0, 0), (0, 0)), (1, 1), (1, 1))]


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_max_pool_is_the_window_maximum(geometry):
    c, slides = pool_circuit("max", *geometry)
    x = np.random.default_rng(7).integers(-40, 41, c.n_inputs).tolist()
    fails, inst = checked(c, x)
    assert fails == [] and inst == [int(w.max()) for w in windows(x, *geometry, slides)]


@pytest.mark.parametrize("normalized", [False, True])
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_sumpool_is_the_window_sum(geometry, normalized):
    from ezkl_amd import ezkl_layout as EL
    c, slides = pool_circuit("sum", *geometry, normalized=normalized)
    x = np.random.default_rng(8).integers(-40, 41, c.n_inputs).tolist()
    fails, inst = checked(c, x)
    sums = [int(w.sum()) for w in windows(x, *geometry, slides)]
    size = geometry[5][0] * geometry[5][1]
    assert fails == [] and inst == ([EL.round_div(s, size) for s in sums] if normalized else sums)


def test_sumpool_assigns_its_unit_kernel_once():
    from ezkl_amd import ezkl_layout as EL
    c, _ = pool_circuit("sum", 2, 4, 5, ((0, 0), (0, 0)), (1, 1), (2, 2))
    reg = c.synthesize(list(range(40)))
    ones = [cell for v, cell in reg.const_order if v == 1]
    assert len(ones) == 1, "one first cell for the constant one: every other unit cell is a copy"


# ---- the classifier --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pool", ["max", "sum"])
def test_the_pool_classifier_proves_its_forward_pass(pool):
    from ezkl_amd import ezkl_layout as EL
    c = EL.PoolClassifierCircuit(10, 2, 12000, pool=pool)
    rng = np.random.default_rng(3)
    x0, x = rng.integers(0, 16, c.n_inputs), rng.integers(0, 16, c.n_inputs)
    fails, inst = checked(c.fresh(), x, key_x=x0)
    assert fails == []
    assert inst == c.model(x) and len(inst) == c.classes + 1
    assert 0 <= inst[-1] < c.classes and inst[inst[-1]] == max(inst[:-1])
