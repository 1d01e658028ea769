"""The claim rules of `recip` and `sqrt` (ezkl_layout.recip_claim / sqrt_claim) and the ops built on them -- `recip`, `sqrt`, `rsqrt`, `max`,
`percent`, `softmax`, `mean_of_squares` (ezkl_layout.BaseRegion, after layouts.rs:114-143, :300-505, :3022-3035, :5390-5413, :6632-6711).

The rules: against brute force over +-3 around the claim with the two inequalities of `optimum_convex_function`, and against a restatement
of the reference's f64 formulas (tensor/ops.rs `recip` :2353-2370, `sqrt` :1844-1852) in Python floats, which they equal everywhere but at
exact positive ties of the reciprocal.  The ops: NormCircuit at k = 9, softmax and layer norm, under the mock prover -- satisfied; the
claimed reciprocal or root moved by one is reported; a softmax row whose exp-sum is a positive tie is satisfied with the engine's claim
and reported with the f64 value; a zero input of `recip` takes zero_inverse."""
import math
import random

import numpy as np
import pytest

SCALE_PAIRS = [(1, 1), (1, 2), (128, 128), (128, 128 ** 2), (2 ** 7, 2 ** 14), (2 ** 10, 2 ** 20), (2 ** 12, 2 ** 24)]


def f64_round(v):
    """f64::round: half away from zero"""
    return int(math.copysign(math.floor(abs(v) + 0.5), v))


def f64_recip(x, input_scale, output_scale):
    """tensor::ops::nonlinearities::recip for x != 0, operation by operation in f64"""
    rescaled = float(x) / float(input_scale)
    return f64_round(float(output_scale) * (1.0 / rescaled))


def f64_sqrt(x, scale):
    """tensor::ops::nonlinearities::sqrt for x >= 0, operation by operation in f64"""
    return f64_round(float(scale) * math.sqrt(float(x) / float(scale)))


def accepted_recip(x, S, around):
    """the integers within 3 of `around` that satisfy f(y) <= f(y + 1) and f(y) < f(y - 1) for f(y) = |y * x - S|"""
    f = lambda y: abs(y * x - S)
    return [y for y in range(around - 3, around + 4) if f(y) <= f(y + 1) and f(y) < f(y - 1)]


def accepted_sqrt(T, around):
    f = lambda y: abs(y * y - T)
    return [y for y in range(max(around - 3, 0), around + 4) if f(y) <= f(y + 1) and f(y) < f(y - 1)]      # (`abs` holds the claim to y >= 0)


def test_the_reciprocal_claim_is_the_one_value_the_gates_accept():
    from ezkl_amd import ezkl_layout as EL
    rng = random.Random(1)
    for si, so in SCALE_PAIRS:
        S = si * so
        xs = [x for x in range(-70, 71) if x] + [rng.choice([-1, 1]) * rng.randrange(1, 1 << 30) for _ in range(2000)] + [rng.randrange(1, 4 * S + 2) for _ in range(2000)]
        xs += [S, -S, 2 * S, -2 * S, 2 * S - 1, 2 * S + 1, -(2 * S + 1)]
        for x in xs:
            y = EL.recip_claim(x, S, 7)
            assert accepted_recip(x, S, y) == [y], (x, S, y)
    assert EL.recip_claim(0, 512, 8192) == 8192 and EL.recip_claim(2, 1, 0) == 0 and EL.recip_claim(-2, 1, 0) == -1 and EL.recip_claim(4, 2, 0) == 0
    assert EL.recip_claim((1 << 62) - 1, (1 << 62) - 1, 0) == 1 and EL.recip_claim(-(1 << 62) + 1, 1, 0) == 0
    for x in (1 << 62, -(1 << 62)):
        with pytest.raises(AssertionError, match=EL.RECIP_ERROR):
            EL.recip_claim(x, 1, 0)
    assert EL.RECIP_ERROR == "reciprocal operand beyond 62 bits" and EL.SQRT_ERROR == "square-root operand outside the exact range"


def test_the_reciprocal_claim_is_the_f64_value_except_at_positive_ties():
    from ezkl_amd import ezkl_layout as EL
    si, so = 2 ** 7, 2 ** 14
    S = si * so
    assert S == 1 << 21
    rng = random.Random(2)
    for sign in (1, -1):
        xs = [sign * rng.randrange(1, 1 << 30) for _ in range(20000)] + [sign * v for v in (1, 2, S, 2 * S, 4 * S, (1 << 30) - 1)]
        ties = [x for x in xs if x > 0 and (2 * S) % x == 0 and S % x != 0]
        assert len(ties) <= len(xs) // 100 and set(ties) <= {1 << 22}, "only x = 2^22 divides 2S = 2^22 without dividing S"
        for x in xs:
            if x not in ties:
                assert EL.recip_claim(x, S, 0) == f64_recip(x, si, so), x
        for x in ties:                                                   # the f64 rounds the tie up; the gates take the smaller one
            assert f64_recip(x, si, so) == EL.recip_claim(x, S, 0) + 1 == 1 and accepted_recip(x, S, 1) == [0]
    assert f64_recip(-(1 << 22), si, so) == EL.recip_claim(-(1 << 22), S, 0) == -1, "a negative tie: both round away from zero"


def test_the_root_claim_is_the_one_value_the_gates_accept_and_the_f64_value():
    from ezkl_amd import ezkl_layout as EL
    rng = random.Random(3)
    for scale in (1, 128, 2 ** 12):
        xs = list(range(-5, 3000)) + [rng.randrange(1 << 36) for _ in range(3000)]
        for x in xs:
            y = EL.sqrt_claim(x, scale)
            assert accepted_sqrt(x * scale, y) == [y], (x, scale, y)
            if x >= 0:
                assert y == f64_sqrt(x, scale), (x, scale)
            else:
                assert y == 0
    top = (1 << 31) - 1
    assert [EL.sqrt_claim(t, 1) for t in (top * top, top * top + top, top * top + top + 1, (1 << 62) - 1)] == [top, top, top + 1, top + 1]
    assert EL.sqrt_claim(-(1 << 62) + 1, (1 << 31) - 1) == 0
    for x, scale in ((1 << 62, 1), (-(1 << 62), 1), (1 << 55, 128), ((1 << 31) + 2, (1 << 31) - 1)):      # beyond 62 bits, or T >= 2^62
        with pytest.raises(AssertionError, match=EL.SQRT_ERROR):
            EL.sqrt_claim(x, scale)
    assert EL.sqrt_claim((1 << 31) + 1, (1 << 31) - 1) == EL.sqrt_claim((1 << 62) - 1, 1) == 1 << 31, "the largest T of that scale"


# ---- the ops under the mock prover -----------------------------------------------------------------------------------------------------------
ROWS, LENGTH = 2, 4
VARIANTS = ["softmax", "layer_norm"]


def circuit(variant, **kw):
    from ezkl_amd import ezkl_layout as EL
    return EL.NormCircuit(9, 2, 3000, ROWS, LENGTH, layer_norm=(variant == "layer_norm"), **kw)


def inputs(seed):
    """values in [-12, 12] (at the input scale 8: +-1.5), the first value again at the end of its row"""
    x = np.random.default_rng(seed).integers(-12, 13, ROWS * LENGTH).tolist()
    x[LENGTH - 1] = x[0]
    return x


def laid_out(c, x):
    from ezkl_amd import ezkl_layout as EL
    reg = EL.BaseRegion(c.gc)
    outs = c.layout(reg, [EL.Val(int(v) % EL.R) for v in x], EL.Val)
    reg.finish(c.gc.const_cols)
    n = 1 << c.k
    return [list(reg.advice.get(col.index) or [0] * n) for col in c.gc.cs.advice], [[v.v for v in outs]], reg


@pytest.fixture(scope="module")
def keys():
    """(constraint system, fixed columns, copies) per (variant, circuit options), made once"""
    made = {}

    def get(variant, **kw):
        key = (variant, tuple(sorted(kw.items())))
        if key not in made:
            cs, fixed, copies, _ = circuit(variant, **kw).keygen_inputs(inputs(1) if not kw else [0] * (ROWS * LENGTH))
            made[key] = (cs, [list(f) for f in fixed], list(copies))
        return made[key]
    return get


def check(keys, variant, adv, inst, **kw):
    from oracle import mock_prover as MP
    cs, fixed, copies = keys(variant, **kw)
    return MP.check(cs, adv, fixed, inst, copies, max_failures=64)


def softmax_model(row, si, so):
    """the integer forward pass of one softmax row"""
    from ezkl_amd import ezkl_layout as EL
    ex = [int(math.floor(si * math.exp((v - max(row)) / si) + 0.5)) for v in row]
    return [e * EL.recip_claim(sum(ex), si * so, 0) for e in ex]


def layer_norm_model(row, si, so, zero_inverse):
    """the integer forward pass of one layer-norm row"""
    from ezkl_amd import ezkl_layout as EL
    mean = EL.round_div(sum(row), len(row))
    centred = [v - mean for v in row]
    root = EL.sqrt_claim(EL.round_div(sum(d * d for d in centred), len(row)), si)
    return [EL.round_div(d * EL.recip_claim(root, si * so, zero_inverse), si) for d in centred]


@pytest.mark.parametrize("variant", VARIANTS)
def test_the_mock_prover_accepts_the_layout(keys, variant):
    from ezkl_amd import ezkl_layout as EL
    for seed in (1, 2):                                              # the keys were made on seed 1: the layout does not depend on the values
        x = inputs(seed)
        adv, inst = circuit(variant).witness(x)
        assert check(keys, variant, adv, inst) == []
        got = [EL.signed(v) for v in inst[0]]
        if variant == "softmax":
            assert got == [v for i in range(ROWS) for v in softmax_model(x[i * LENGTH:(i + 1) * LENGTH], 8, 64)]
            assert all(abs(sum(got[i * LENGTH:(i + 1) * LENGTH]) - 8 * 64) <= 8 * LENGTH for i in range(ROWS)), "a row sums to one at the scale 512"
        else:
            assert got == [v for i in range(ROWS) for v in layer_norm_model(x[i * LENGTH:(i + 1) * LENGTH], 8, 64, 8192)]


def _moved(name, by):
    """ezkl_layout with one claim rule answering `by` more than it should (a prover that cheats consistently: every copy follows)"""
    from ezkl_amd import ezkl_layout as EL
    true = getattr(EL, name)
    return lambda *a: true(*a) + by


@pytest.mark.parametrize("by", [1, -1])
@pytest.mark.parametrize("variant", VARIANTS)
def test_a_claimed_reciprocal_moved_by_one_is_reported(keys, monkeypatch, variant, by):
    from ezkl_amd import ezkl_layout as EL
    x = inputs(3)
    monkeypatch.setattr(EL, "recip_claim", _moved("recip_claim", by))
    adv, inst, _ = laid_out(circuit(variant), x)
    fails = check(keys, variant, adv, inst)
    assert fails and all(f.startswith("copy") for f in fails), "enforce_equality of the optimum with one: %s" % fails[:3]


@pytest.mark.parametrize("by", [1, -1])
def test_a_claimed_root_moved_by_one_is_reported(keys, monkeypatch, by):
    from ezkl_amd import ezkl_layout as EL
    x = inputs(4)
    honest = circuit("layer_norm").witness(x)[0]
    moved = _moved("sqrt_claim", by)
    monkeypatch.setattr(EL, "sqrt_claim", lambda s, scale: max(moved(s, scale), 0))
    adv, inst, _ = laid_out(circuit("layer_norm"), x)
    assert adv != honest, "the roots of these rows are above zero: the claim did move"
    fails = check(keys, "layer_norm", adv, inst)
    assert fails and all(f.startswith("copy") for f in fails), fails[:3]


TIE = dict(input_scale=2, output_scale=1, eps=1.0 / 64)


def test_a_positive_tie_is_satisfied_with_the_engines_claim_and_reported_with_the_f64_value(keys, monkeypatch):
    """scales 2 and 1: S = 2, and a row of two zeros among very negative ones has the exp-sum 2 + 2 = 4 = 2S.  |0 * 4 - 2| = |1 * 4 - 2|: the
    gates take the smaller claim, 0; the f64 formula says round(1 / (4 / 2)) = round(0.5) = 1, which `less(f(y), f(y - 1))` refuses"""
    from ezkl_amd import ezkl_layout as EL
    x = [0, -200, 0, -200, 5, 5, -200, -200]
    assert f64_recip(4, 2, 1) == 1 and EL.recip_claim(4, 2, 0) == 0
    adv, inst = circuit("softmax", **TIE).witness(x)
    assert check(keys, "softmax", adv, inst, **TIE) == [] and inst == [[0] * 8]
    monkeypatch.setattr(EL, "recip_claim", lambda s, S, zi: zi if s == 0 else f64_recip(s, 2, 1))
    adv, inst, _ = laid_out(circuit("softmax", **TIE), x)
    assert [EL.signed(v) for v in inst[0]] == [2, 0, 2, 0, 2, 2, 0, 0]
    fails = check(keys, "softmax", adv, inst, **TIE)
    assert fails and all(f.startswith("copy") for f in fails), fails[:3]


def test_a_zero_input_of_recip_takes_zero_inverse(keys):
    """a constant row has the mean square 0, the root 0, and `recip` of 0 is round(output_scale / eps) = 64 * 128; the other row is honest"""
    from ezkl_amd import ezkl_layout as EL
    x = [7, 7, 7, 7, 3, -4, 9, 0]
    c = circuit("layer_norm")
    adv, inst, reg = laid_out(c, x)
    assert check(keys, "layer_norm", adv, inst) == []
    assert EL.zero_recip(64, 1.0 / 128) == 8192 and inst[0][:4] == [0, 0, 0, 0] and any(inst[0][4:])
    assert any(8192 in col for col in adv), "the claimed reciprocal of the zero root"
    seen = []

    class Spy(EL.BaseRegion):
        def recip(self, vals, *a):
            out = EL.BaseRegion.recip(self, vals, *a)
            seen.extend((EL.signed(v.v), EL.signed(o.v)) for v, o in zip(vals, out))
            return out
    c.layout(Spy(c.gc), [EL.Val(v % EL.R) for v in x], EL.Val)
    assert seen[0] == (0, 8192) and seen[1][0] > 0 and seen[1][1] == EL.recip_claim(seen[1][0], 512, 8192)
    # and a claim other than zero_inverse for the zero is reported
    real = EL.recip_claim
    try:
        EL.recip_claim = lambda s, S, zi: real(s, S, zi) - (s == 0)
        adv, inst, _ = laid_out(circuit("layer_norm"), x)
    finally:
        EL.recip_claim = real
    assert check(keys, "layer_norm", adv, inst)


def test_the_small_ops():
    from ezkl_amd import ezkl_layout as EL

    def placed(values):
        """a fresh region of the softmax circuit with `values` assigned on its first input VarTensor"""
        reg = EL.BaseRegion(circuit("softmax").gc)
        reg.decomp = (128, 2)
        vals = reg.assign(reg.inputs[0], [EL.Val(v % EL.R) for v in values])
        reg.increment(len(vals))
        return reg, vals
    reg, vals = placed((5, -2, 9, 0))
    assert EL.signed(reg.max(vals).v) == 9 and EL.signed(reg.min(vals).v) == -2 and reg.shuffle_index == 2
    assert [v.v for v in reg.not_([EL.Val(1), EL.Val(0), EL.Val(1)])] == [0, 1, 0]
    assert [v.v for v in reg.mean_of_squares([vals, vals[::-1]])] == [EL.round_div(25 + 4 + 81, 4)] * 2
    reg, doc = placed((2, 15, 2, 1, 1, 0))                            # layouts.rs:3011-3019
    assert [v.v for v in reg.mean_of_squares([doc[:3], doc[3:]])] == [78, 1]
    reg, nine = placed((1, 2, 3, 2, 3, 4, 3, 4, 9))                   # layouts.rs:400-405: sqrt at scale 1
    assert [v.v for v in reg.sqrt(nine, 1)] == [1, 1, 2, 1, 2, 2, 2, 2, 3]
    reg, six = placed((2, 1, 2, 7, 1, 1))                             # ops.rs:2344-2350: recip at scales (1, 2)
    assert [v.v for v in reg.recip(six, 1, 2, 1.0 / 64)] == [1, 2, 1, 0, 2, 2]
    reg, five = placed((1, 2, 3, 4, 5))                               # layouts.rs:474-479 lists 1 throughout for rsqrt at scales (1, 1): from 3 on the root is 2,
    assert [v.v for v in reg.rsqrt(five, 1, 1, 1.0 / 64)] == [1, 1, 0, 0, 0]      # the tie x = 2S, where the f64 value 1 is not what the gates take
