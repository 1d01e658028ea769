"""`BaseRegion.sort_ascending` / `topk` / `topk_axes` (ezkl_layout.py, after layouts.rs:1124-1361 and `shuffles`, :1624-1760) under the mock
prover: SortTopkCircuit is satisfied in all three collision modes on inputs with duplicates, from one element to a sorted run that crosses
the top of a column; a sort laid out consistently from a wrong order, a wrong claimed index, or a sorted cell changed where the argument
does not read it is reported."""
import numpy as np
import pytest

MODES = ["unsorted", "smallest_index_first", "largest_index_first"]
# (logrows, inner columns, length): k = 9 has 506 usable rows; with one inner column the second sorted run of 19 starts below the top of a
# column and ends above it
SHAPES = [(9, 2, 1), (9, 2, 2), (9, 2, 3), (9, 2, 8), (10, 2, 13), (9, 1, 19)]
CROSSING = (9, 1, 19)
K_TOP = 3


def circuit(k, w, length, mode, largest=True):
    from ezkl_amd import ezkl_layout as EL
    return EL.SortTopkCircuit(k, w, 3000, length, min(K_TOP, length), largest, mode, 16, 2)


def inputs(length, seed):
    """values in [-100, 100] with duplicates: the first value again at the end, and -- from eight on -- a run of three equal ones"""
    x = np.random.default_rng(seed).integers(-100, 101, length).tolist()
    x[-1] = x[0]
    if length >= 8:
        x[2] = x[4] = x[5]
    return x


def laid_out(c, x, region=None):
    """(advice columns, instance, region) of the circuit's layout on `region` (a BaseRegion subclass: a prover that cheats consistently)"""
    from ezkl_amd import ezkl_layout as EL
    reg = (region or EL.BaseRegion)(c.gc)
    outs = c.layout(reg, [EL.Val(int(v) % EL.R) for v in x], EL.Val)
    reg.finish(c.gc.const_cols)
    n = 1 << c.k
    return [list(reg.advice.get(col.index) or [0] * n) for col in c.gc.cs.advice], [[v.v for v in outs]], reg


def sorted_cells(reg, c):
    """the cells of the full sort's run on the first input VarTensor: what the instance column is tied to after the top-k"""
    return [a for a, b in reg.copies if b[0] == "inst"][min(K_TOP, c.n_inputs):]


@pytest.fixture(scope="module")
def keys():
    """(constraint system, fixed columns, copies) per (shape, mode), made once"""
    made = {}

    def get(shape, mode):
        if (shape, mode) not in made:
            c = circuit(*shape, mode)
            cs, fixed, copies, _ = c.keygen_inputs(inputs(shape[2], 1))
            made[shape, mode] = (cs, [list(f) for f in fixed], list(copies))
        return made[shape, mode]
    return get


def check(keys, shape, mode, adv, inst, **kw):
    from oracle import mock_prover as MP
    cs, fixed, copies = keys(shape, mode)
    return MP.check(cs, adv, fixed, inst, copies, **kw)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_the_mock_prover_accepts_the_layout(keys, shape, mode):
    from ezkl_amd import ezkl_layout as EL
    length = shape[2]
    for seed in (1, 2):                                              # the keys were made on seed 1: the layout does not depend on the values
        x = inputs(length, seed)
        c = circuit(*shape, mode)
        adv, inst = c.witness(x)
        assert check(keys, shape, mode, adv, inst) == []
        assert [EL.signed(v) for v in inst[0]] == sorted(x, reverse=True)[:min(K_TOP, length)] + sorted(x)
    smallest = circuit(*shape, mode, largest=False)
    assert [EL.signed(v) for v in smallest.witness(x)[1][0]] == sorted(x)[:min(K_TOP, length)] + sorted(x)
    if shape == CROSSING:
        _, _, reg = laid_out(circuit(*shape, mode), x)
        run = sorted_cells(reg, c)
        assert len({cell[1] for cell in run}) == 2 and run[0][2] > run[-1][2], "the sorted run starts in one column and ends at the top of the next"


def test_the_order_is_by_value_then_position():
    from ezkl_amd import ezkl_layout as EL
    reg = EL.BaseRegion(circuit(9, 2, 8, "unsorted").gc)
    vals = [EL.Val(v) for v in (5, -2, 5, 0, -2, 5)]
    assert reg._sorted(vals, "unsorted") == reg._sorted(vals, "smallest_index_first") == ([EL.R - 2, EL.R - 2, 0, 5, 5, 5], [1, 4, 3, 0, 2, 5])
    assert reg._sorted(vals, "largest_index_first") == ([EL.R - 2, EL.R - 2, 0, 5, 5, 5], [4, 1, 3, 5, 2, 0])
    one = [EL.Val(-9, ("adv", 0, 0))]
    srt, idx = reg.sort_ascending(one, "largest_index_first")
    assert srt == one and (idx[0].v, idx[0].const) == (0, True) and reg.linear == 0 and not reg.advice, "length 1: its input and a zero, no cell written"


def _cheat(tamper):
    """a BaseRegion whose `_sorted` answers tamper(values, positions) for the circuit's full sort (the second of the region)"""
    from ezkl_amd import ezkl_layout as EL

    class Cheat(EL.BaseRegion):
        def _sorted(self, vals, mode):
            values, positions = EL.BaseRegion._sorted(self, vals, mode)
            return tamper(list(values), list(positions)) if self.shuffle_index == 1 else (values, positions)
    return Cheat


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(9, 2, 8), CROSSING])
def test_a_wrong_order_laid_out_consistently_is_reported(keys, shape, mode):
    """two sorted cells swapped, with their claimed indices and every copy of them: the permutation argument and the copies hold, the
    ordering constraint does not"""
    x = inputs(shape[2], 3)
    at = next(i for i in range(len(x) - 1) if sorted(x)[i] != sorted(x)[i + 1])

    def swap(values, positions):
        values[at], values[at + 1] = values[at + 1], values[at]
        positions[at], positions[at + 1] = positions[at + 1], positions[at]
        return values, positions
    adv, inst, _ = laid_out(circuit(*shape, mode), x, _cheat(swap))
    fails = check(keys, shape, mode, adv, inst)
    assert fails and all(f.startswith("copy") for f in fails), "enforce_equality of the comparison with one: %s" % fails[:3]


@pytest.mark.parametrize("mode", MODES)
def test_the_claimed_indices_of_equal_values_are_held_to_the_mode(keys, mode):
    """the positions of two equal values the other way round: still a permutation, and sorted by value -- the unsorted mode takes it, the
    indexed modes take only their own order"""
    shape = (9, 2, 8)
    x = inputs(8, 4)
    srt = sorted(x)
    at = next(i for i in range(7) if srt[i] == srt[i + 1])

    def swap(values, positions):
        positions[at], positions[at + 1] = positions[at + 1], positions[at]
        return values, positions
    adv, inst, _ = laid_out(circuit(*shape, mode), x, _cheat(swap))
    fails = check(keys, shape, mode, adv, inst)
    assert (fails == []) == (mode == "unsorted"), fails[:3]


@pytest.mark.parametrize("mode", MODES)
def test_a_changed_claimed_index_is_reported(keys, mode):
    """a claimed index that is another element's: the input side (input_j, shuffle index, j) is no row of the table"""
    shape = (9, 2, 8)
    x = inputs(8, 5)

    def wrong(values, positions):
        positions[3] = positions[6]
        return values, positions
    adv, inst, _ = laid_out(circuit(*shape, mode), x, _cheat(wrong))
    fails = check(keys, shape, mode, adv, inst, max_failures=64)
    assert any(f.startswith("lookup") for f in fails), fails[:3]
    # and changed in its cell alone, after an honest layout: the table's third column, row of the second sort's entry 3
    c = circuit(*shape, mode)
    adv, inst, reg = laid_out(c, x)
    col = c.gc.advices[5].inner[0][0].index
    adv[col][8 + 3] = (adv[col][8 + 3] + 1) % 8
    assert check(keys, shape, mode, adv, inst, max_failures=64)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(9, 2, 8), CROSSING])
def test_a_sorted_cell_changed_beside_the_table_is_reported_by_its_copy(keys, shape, mode):
    """the sorted value on the first input VarTensor changed while the table side keeps the true one: the argument still holds, the copy
    between the two cells does not"""
    x = inputs(shape[2], 6)
    c = circuit(*shape, mode)
    adv, inst, reg = laid_out(c, x)
    run = sorted_cells(reg, c)
    _, col, row = run[len(run) - 1]                                   # the last sorted cell: at the top of the next column in the crossing shape
    adv[col][row] = adv[col][row] + 1
    table = c.gc.advices[3].inner[0][0].index
    fails = check(keys, shape, mode, adv, inst, max_failures=256)
    assert any(f.startswith("copy") and "adv%d," % table in f and "adv%d,%d" % (col, row) in f for f in fails), fails[:5]


class TwoRowsCircuit:
    """`topk_axes` over the two rows of one input vector: instance = the top k of the first row, then of the second"""

    def __init__(self, length, k_top, largest=True):
        from ezkl_amd import ezkl_circuit as EC
        self.k, self.w, self.n_inputs, self.k_top, self.length, self.largest = 9, 1, 2 * length, k_top, length, largest
        self.settings = EC.GraphSettings(9, 1, 2000, total_const_size=4, required_range_checks=[(-1, 1), (0, 15)], model_instance_shapes=[[1, 2 * k_top]],
                                         total_shuffle_col_size=2 * length, num_shuffles=1)
        self.gc = EC.GraphConfig(self.settings)

    def layout(self, reg, inputs, param):
        reg.decomp = (16, 2)
        vals = reg.assign(reg.inputs[0], inputs)
        reg.increment(len(vals))
        tops = reg.topk_axes([vals[:self.length], vals[self.length:]], self.k_top, self.largest)
        outs = tops[0] + tops[1]
        reg.constrain_instance(outs, self.gc.instance)
        return outs

    def plan_identity(self):
        return b"two rows %d %d %d" % (self.length, self.k_top, self.largest)


def test_the_doc_example_of_topk_axes():
    """layouts.rs:1332-1341: rows [2, 15, 2] and [1, 1, 0], k = 2, largest -> [15, 2] and [1, 1]"""
    c = TwoRowsCircuit(3, 2)
    adv, inst, reg = laid_out(c, [2, 15, 2, 1, 1, 0])
    assert inst == [[15, 2, 1, 1]] and reg.shuffle_index == 2, "one shuffle index per sort of the region"
    _, inst, _ = laid_out(TwoRowsCircuit(3, 2, largest=False), [2, 15, 2, 1, 1, 0])
    assert inst == [[2, 2, 0, 1]]
    table = c.gc.advices[4].inner[0][0].index
    assert adv[table][:6] == [0, 0, 0, 1, 1, 1], "the shuffle index is the constant of the argument's second coordinate"
