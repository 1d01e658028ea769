"""`BaseRegion.select_elements`, `gather`, `gather_elements`, `one_hot`, `one_hot_axis`, `get_missing_set_elements` and `scatter_elements`
(ezkl_layout.py, after layouts.rs:1363-1442, :1769-1870, :1924-2012 and :2213-2379) under the mock prover: the doc examples of the reference,
1-D and 2-D tensors along both dims, one element, as many elements as cells (an empty complement), the identity and its reverse; a scatter
claim with a scattered value, an untouched value or a missing index changed is reported; a duplicate target takes the later source and has
no witness; one-hot claims with two ones or none are reported; ScatterGatherCircuit proves its integer forward pass."""
import numpy as np
import pytest

from test_pool_layout_cpu import OpCircuit, checked


def scatter_circuit(dims, index_dims, dim):
    n, m = int(np.prod(dims)), int(np.prod(index_dims))
    op = lambda reg, v: reg.scatter_elements(v[:n], dims, v[n:n + m], index_dims, v[n + m:], dim)
    return OpCircuit(n + 2 * m, n, op, sorts=2, sort_rows=2 * n, selects=3, select_rows=3 * n, k=10, capacity=8000)


def scatter_model(x, dims, index_dims, dim):
    n, m = int(np.prod(dims)), int(np.prod(index_dims))
    t = np.array(x[:n], np.int64).reshape(dims)
    np.put_along_axis(t, np.array(x[n:n + m], np.int64).reshape(index_dims), np.array(x[n + m:], np.int64).reshape(index_dims), axis=dim)
    return t.reshape(-1).tolist()


def test_the_doc_example_of_scatter_elements():
    """layouts.rs:2310-2312"""
    fails, inst = checked(scatter_circuit([3], [2], 0), [1, 2, 3] + [0, 2] + [10, 20])
    assert fails == [] and inst == [10, 2, 20]


SCATTERS = [([5], [1], 0, [3]), ([5], [5], 0, [0, 1, 2, 3, 4]), ([5], [5], 0, [4, 3, 2, 1, 0]), ([7], [3], 0, [6, 0, 2]),
            ([3, 4], [2, 4], 0, [2, 0, 1, 1, 0, 2, 2, 0]), ([3, 4], [3, 2], 1, [3, 0, 1, 2, 0, 3]), ([2, 3], [2, 3], 0, [1, 0, 1, 0, 1, 0]), ([4, 1], [1, 1], 0, [2])]


@pytest.mark.parametrize("dims,index_dims,dim,index", SCATTERS)
def test_scatter_elements_is_put_along_axis(dims, index_dims, dim, index):
    n = int(np.prod(dims))
    rng = np.random.default_rng(n + dim)
    x = rng.integers(-40, 41, n).tolist() + index + rng.integers(50, 90, len(index)).tolist()
    fails, inst = checked(scatter_circuit(dims, index_dims, dim), x, key_x=[0] * len(x))
    assert fails == [] and inst == scatter_model(x, dims, index_dims, dim)


def _cheat(method, move):
    """a BaseRegion whose data-dependent step `method` answers move(honest claim)"""
    from ezkl_amd import ezkl_layout as EL
    return type("Cheat", (EL.BaseRegion,), {method: lambda self, *a: move(getattr(EL.BaseRegion, method)(self, *a))})


def _changed(at, to):
    def move(claim):
        claim = list(claim)
        claim[at] = to
        return claim
    return move


X7 = [11, 12, 13, 14, 15, 16, 17] + [6, 0, 2] + [60, 61, 62]            # -> [61, 12, 62, 14, 15, 16, 60]; missing 1, 3, 4, 5


def test_a_tampered_scatter_claim_is_reported():
    c = lambda: scatter_circuit([7], [3], 0)
    fails, inst = checked(c(), X7)
    assert fails == [] and inst == [61, 12, 62, 14, 15, 16, 60]
    fails, inst = checked(c(), X7, region=_cheat("_scattered", _changed(2, 99)), max_failures=64)      # a scattered value: the gather at the index is not the source
    assert inst[2] == 99 and fails and all(f.startswith("copy") for f in fails), fails[:3]
    fails, inst = checked(c(), X7, region=_cheat("_scattered", _changed(3, 99)), max_failures=64)      # an untouched value: (3, 99) is no row of (position, input)
    assert inst[3] == 99 and fails and any("lookup" in f for f in fails), fails[:3]
    fails, inst = checked(c(), X7, region=_cheat("_missing", _changed(1, 2)), max_failures=64)         # a missing index: no permutation of the positions
    assert inst == [61, 12, 62, 14, 15, 16, 60] and fails, "the claimed tensor is right, the argument around it is not"


def test_a_duplicate_target_takes_the_later_source_and_has_no_witness():
    """the rule of `tensor::ops::scatter` -- pinned so that it is documented, not relied on: two elements on one target cannot be a permutation"""
    from ezkl_amd import ezkl_layout as EL
    Val = EL.Val
    c = scatter_circuit([5], [3], 0)
    reg = EL.BaseRegion(c.gc)
    out = reg._scattered([Val(v) for v in (1, 2, 3, 4, 5)], [Val(v) for v in (4, 1, 4)], [Val(v) for v in (70, 71, 72)], [5], [3], 0)
    assert out == [1, 71, 3, 4, 72]
    fails, inst = checked(c, [1, 2, 3, 4, 5] + [4, 1, 4] + [70, 71, 72], max_failures=64)
    assert inst == [1, 71, 3, 4, 72] and fails


def test_scattered_and_one_hot_assert_their_ranges():
    from ezkl_amd import ezkl_layout as EL
    Val = EL.Val
    reg = EL.BaseRegion(scatter_circuit([5], [1], 0).gc)
    base = [Val(v) for v in range(5)]
    assert reg._scattered(base, [Val(4)], [Val(9)], [5], [1], 0) == [0, 1, 2, 3, 9] and reg._one_hot(2, 3) == [0, 0, 1] and reg._one_hot(0, 1) == [1]
    for bad in (-1, 5, 1 << 62, -(1 << 62)):
        with pytest.raises(AssertionError, match=EL.SCATTER_ERROR):
            reg._scattered(base, [Val(bad)], [Val(9)], [5], [1], 0)
        with pytest.raises(AssertionError, match=EL.ONEHOT_ERROR):
            reg._one_hot(bad, 5)
    assert reg._missing([Val(v) for v in (2, 9, -1)], [Val(v) for v in range(5)]) == [0, 1], "a value not in the set deletes nothing; the first 5 - 3 are kept"


# ---- gather ------------------------------------------------------------------------------------------------------------------------------
def test_the_doc_example_of_gather_elements():
    """/root/reference/src/tensor/ops.rs:790-799"""
    op = lambda reg, v: reg.gather_elements(v[:4], [2, 2], v[4:], [2, 2], 1)[0]
    fails, inst = checked(OpCircuit(8, 4, op, selects=1, select_rows=4), [1, 2, 3, 4, 0, 0, 1, 0])
    assert fails == [] and inst == [1, 1, 4, 3]


@pytest.mark.parametrize("dims,dim,picks", [([6], 0, [5, 0, 0, 3, 5]), ([3, 4], 0, [2, 2, 0]), ([3, 4], 1, [3, 1, 1, 0, 2]), ([2, 2, 3], 1, [1, 1, 0])])
def test_gather_with_repeated_and_out_of_order_picks_is_take(dims, dim, picks):
    n = int(np.prod(dims))
    op = lambda reg, v: reg.gather(v[:n], dims, v[n:], dim)
    n_out = n // dims[dim] * len(picks)
    x = np.random.default_rng(n).integers(-40, 41, n).tolist() + picks
    fails, inst = checked(OpCircuit(n + len(picks), n_out, op, selects=1, select_rows=n, capacity=8000, k=10), x, key_x=[0] * len(x))
    assert fails == [] and inst == np.take(np.array(x[:n]).reshape(dims), picks, axis=dim).reshape(-1).tolist()


def test_a_select_elements_is_one_lookup_over_one_table():
    from ezkl_amd import ezkl_layout as EL
    c = OpCircuit(7, 3, lambda reg, v: reg.select_elements(v[:4], v[4:]), selects=1, select_rows=4)
    reg = c.synthesize([30, 31, 32, 33, 3, 0, 3])
    assert [EL.signed(v) for v in c.outputs] == [33, 30, 33] and reg.dynamic_lookup_index == 1 and reg.dyn == 4
    with pytest.raises(AssertionError, match=EL.GATHER_ERROR):
        c.synthesize([30, 31, 32, 33, 3, 4, 3])


# ---- one-hot -----------------------------------------------------------------------------------------------------------------------------
def one_hot_circuit(classes):
    return OpCircuit(1, classes, lambda reg, v: reg.one_hot(v[0], classes), selects=1, select_rows=classes)


@pytest.mark.parametrize("classes", [1, 2, 5])
def test_one_hot_of_the_first_and_the_last_class(classes):
    for s in sorted({0, classes - 1}):
        fails, inst = checked(one_hot_circuit(classes), [s], key_x=[0])
        assert fails == [] and inst == [int(j == s) for j in range(classes)]


def test_a_one_hot_claim_with_two_ones_or_none_is_reported():
    fails, inst = checked(one_hot_circuit(5), [3], region=_cheat("_one_hot", _changed(1, 1)), max_failures=64)
    assert inst == [0, 1, 0, 1, 0] and fails, "the sum is 2"
    fails, inst = checked(one_hot_circuit(5), [3], region=_cheat("_one_hot", _changed(3, 0)), max_failures=64)
    assert inst == [0] * 5 and fails, "the sum is 0"
    fails, inst = checked(one_hot_circuit(5), [3], region=_cheat("_one_hot", lambda claim: claim[1:] + claim[:1]), max_failures=64)
    assert inst == [0, 0, 1, 0, 0] and fails, "one one, at another place: the gather at the index is 0"


def test_one_hot_axis_puts_the_classes_at_the_axis():
    x = [2, 0, 1, 1, 2, 0]
    for dim in (0, 1, 2):
        op = lambda reg, v: reg.one_hot_axis(v, [2, 3], 3, dim)
        fails, inst = checked(OpCircuit(6, 18, op, selects=6, select_rows=18, k=10, capacity=8000), x)
        want = np.moveaxis(np.eye(3, dtype=np.int64)[np.array(x).reshape(2, 3)], -1, dim)
        assert fails == [] and inst == want.reshape(-1).tolist()


# ---- the missing set ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("fullset", [list(range(7)), [40, -3, 12, 7, 0, 99, 5]])
def test_get_missing_set_elements(fullset, ordered):
    from ezkl_amd import ezkl_layout as EL
    full = [EL.Val(v, const=True) for v in fullset]
    op = lambda reg, v: reg.get_missing_set_elements(v, full, ordered)
    x = [fullset[5], fullset[0], fullset[3]]
    fails, inst = checked(OpCircuit(3, 4, op, sorts=2, sort_rows=11, k=10, capacity=8000, decomp=(16, 3)), x)
    rest = [v for v in fullset if v not in x]
    assert fails == [] and inst == (sorted(rest) if ordered else rest), "in the order of the full set, or ascending"


def test_a_value_outside_the_full_set_has_no_witness():
    from ezkl_amd import ezkl_layout as EL
    full = [EL.Val(v, const=True) for v in range(5)]
    op = lambda reg, v: reg.get_missing_set_elements(v, full, False)
    fails, inst = checked(OpCircuit(2, 3, op, sorts=1, sort_rows=5), [1, 9], max_failures=64)
    assert inst == [0, 2, 3] and fails, "9 deletes nothing, the first 5 - 2 of what remains are kept, and the permutation cannot hold"


# ---- the circuit -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_scatter_gather_circuit_proves_its_forward_pass(seed):
    from ezkl_amd import ezkl_layout as EL
    from test_witness_plan_scatter_cpu import inputs
    c = EL.ScatterGatherCircuit(10, 2, 6000)
    x = inputs(c, seed)
    fails, inst = checked(c.fresh(), x, key_x=inputs(c, 0))
    assert fails == []
    assert inst == c.model(x) and len(inst) == c.picks * c.cols + c.rows and sum(inst[-c.rows:]) == 1 and inst[-c.rows + x[-c.picks]] == 1
