"""A circuit family states its fields ONCE, in `config()`: the constructor's keyword arguments, read off the live attributes.  Without a
device, over every class that has one, at the smallest shapes of the existing case files: `fresh()` and `execute.describe` carry every
field -- a field mutated after construction reaches the fresh circuit and (but for the listed exceptions) its plan identity --, a
description round-trips to an equal `config()`, `params_hash` is the documented prefix, the identity and the table bytes, and a circuit
with second-phase advice that does not declare its einsums is still refused by `record_plan`."""
import hashlib
import inspect
import json
import struct

import numpy as np
import pytest

import batch_mlp_cases as BF
import execute_family_cases as F
import visibility_cases as VC


def _mlp():
    from ezkl_amd import ezkl_layout as EL
    return EL.MlpCircuit(9, 2, [VC.WEIGHTS, [[1, 0, -1, 2], [0, 2, 1, 0]]], [VC.BIASES, [3, -4]], VC.BASE, VC.LEGS, rebase=[1, 2], relu_last=False)


def _layout_class(name, *args):
    def make():
        from ezkl_amd import ezkl_layout as EL
        return getattr(EL, name)(*args)
    return make


# name -> (make the circuit, the family `execute.describe` writes it as or None)
CASES = {
    "mlp": (_mlp, None),
    "conv_k6": (F.conv_k6, "conv"),
    "norm_softmax": (lambda: F.norm(False), "norm"),
    "norm_layer_norm": (lambda: F.norm(True), "norm"),
    "pool_max": (lambda: F.pool("max"), "pool_classifier"),
    "scatter_gather": (_layout_class("ScatterGatherCircuit", 10, 2, 6000), None),
    "attention": (BF.attention, "attention"),
    "batch_tiny": (lambda: BF.batch(BF.TINY), "mlp_batch"),
    "batch_ragged": (lambda: BF.batch(BF.RAGGED), "mlp_batch"),                  # (rebase divisors: the description states its scales)
    "sort_topk": (_layout_class("SortTopkCircuit", 9, 2, 3000, 8, 3, True, "unsorted", 16, 2), None),
    "sum_prod_layout": (_layout_class("SumProdLayoutCircuit", 6, 2, 67, 5), None),
    "sum_prod": (_layout_class("SumProdCircuit", 6, 2, 67), None),               # (no `layout`: no plan identity to compare)
}
# where a constructor parameter is kept under another name
ATTRIBUTES = dict(logrows="k", num_inner_cols="w", decomp_base="base", decomp_legs="legs", out_channels="oc", batch="m",
                  total_assignments="settings.total_assignments", total_const_size="settings.total_const_size")
LENGTH_IS_N_INPUTS = ("sort_topk", "sum_prod_layout")
# the options `plan_identity()` deliberately leaves out, per class: a fresh circuit with one of them changed keeps its identity
NOT_IN_IDENTITY = {
    "mlp": {"total_assignments", "total_const_size"},   # the settings' counts: a plan addresses cells, and its pinned bytes predate both
    "conv_k6": {"seed",                                 # all four arrays it seeds are in the identity themselves
                "lookup_range"},                        # the Div table over it is hashed by params_hash with the other static tables (checked below)
    "pool_max": {"seed"},                               # as the conv circuit's
    "attention": {"seed"},                              # Wq, Wk, Wv are in the identity; the default INPUT it also seeds is no part of a plan
}
# a mutation of one of these alone may leave a circuit its constructor refuses -- the given arrays have the old shape, an einsum layout
# takes one inner column: the refusal shows that `fresh()` carried the field
SETS_A_SHAPE = {"kernel", "out_channels", "stride", "classes", "pool_size", "pool_stride", "e", "d", "n_inputs", "num_inner_cols"}


def _attribute(name, key):
    return "n_inputs" if key == "length" and name in LENGTH_IS_N_INPUTS else ATTRIBUTES.get(key, key)


def _get(c, path):
    for part in path.split("."):
        c = getattr(c, part)
    return c


def _set(c, path, value):
    *head, last = path.split(".")
    setattr(_get(c, ".".join(head)) if head else c, last, value)


def _plain(v):
    """arrays and tuples as (nested) lists: what a description holds"""
    return v.tolist() if isinstance(v, np.ndarray) else [_plain(x) for x in v] if isinstance(v, (tuple, list)) else v


def _same(a, b):
    return set(a) == set(b) and all(_plain(a[key]) == _plain(b[key]) and type(_plain(a[key])) is type(_plain(b[key])) for key in a)


def _bumped(v):
    """a nested list with one added to its first entry"""
    return [_bumped(v[0])] + list(v[1:]) if isinstance(v[0], list) else [v[0] + 1] + list(v[1:])


def _mutated(c, key, v):
    if isinstance(v, np.ndarray):
        return v + 1
    if isinstance(v, bool):
        return not v
    if key in ("capacity", "total_assignments"):                                # past a block of the model columns: another configuration
        return (v or 0) + (2 * c.w << c.k)
    if key == "visibility":
        return ("Public", "Private", "Public")
    if key == "lookup_range":
        return (v[0] - 1, v[1])
    if key == "eps":
        return v * 2
    if key == "pool":
        return "sum" if v == "max" else "max"
    if key == "mode":
        return "largest_index_first"
    if isinstance(v, list):
        return _bumped(v)
    assert isinstance(v, int), (key, v)
    return v + 1


def _settings(c):
    s = c.gc.settings
    return (s.logrows, s.num_inner_cols, s.total_assignments, s.total_const_size, s.required_range_checks, [n for n, _ in s.required_lookups], s.lookup_range,
            s.model_instance_shapes, s.total_dynamic_col_size, s.num_dynamic_lookups, s.total_shuffle_col_size, s.num_shuffles, len(c.gc.cs.advice))


def _identity(c):
    return c.plan_identity() if hasattr(c, "plan_identity") else None


@pytest.mark.parametrize("name", list(CASES))
def test_config_is_the_constructor_s_arguments_and_builds_the_same_circuit(name):
    c = CASES[name][0]()
    cfg = c.config()
    assert set(cfg) == set(inspect.signature(type(c).__init__).parameters) - {"self"}          # a parameter cannot be forgotten here
    for again in (type(c)(**cfg), c.fresh()):
        assert type(again) is type(c) and again is not c and again.gc.cs is not c.gc.cs
        assert _identity(again) == _identity(c) and _settings(again) == _settings(c) and _same(again.config(), cfg)


@pytest.mark.parametrize("name", list(CASES))
def test_every_field_mutated_alone_reaches_config_fresh_and_the_plan_identity(name):
    from ezkl_amd import witness_plan as WP
    make = CASES[name][0]
    for key in make().config():
        c = make()
        before, identity, attribute = c.config(), _identity(c), _attribute(name, key)
        _set(c, attribute, _mutated(c, key, before[key]))
        after = c.config()
        assert _plain(after[key]) != _plain(before[key]), key                                # `config` reads the attribute as it is now
        assert _same({k: v for k, v in after.items() if k != key}, {k: v for k, v in before.items() if k != key}), key
        try:
            fresh = c.fresh()
        except (ValueError, AssertionError):
            assert key in SETS_A_SHAPE and c.plan_identity() != identity, key
            continue
        assert _same(fresh.config(), after), key
        if identity is None:
            continue
        if key in NOT_IN_IDENTITY.get(name, ()):
            assert fresh.plan_identity() == identity, key
        else:
            assert fresh.plan_identity() != identity, key
        if name == "conv_k6" and key == "lookup_range":
            assert WP.params_hash(fresh) != WP.params_hash(make())


@pytest.mark.parametrize("name", [name for name, (_, family) in CASES.items() if family])
def test_a_description_is_config_split_into_run_args_and_fields(tmp_path, name):
    from ezkl_amd import execute as X
    make, family = CASES[name]
    c = make()
    cfg, d = c.config(), X.describe(c, input_scale=3, output_scale=5)
    assert d["model"] == family and list(d)[:2] == ["model", "run_args"]
    written = (set(d) - {"model", "run_args"}) | set(d["run_args"])
    # beyond config: the two scales of a witness file, which are no field of a circuit (the norm and attention circuits have fields of
    # those names too, at the top level).  Of config, a description leaves out the seed -- every array it seeds is written -- and, of
    # a batched MLP that rescales nothing, the divisors (all 1): the MLP description's rule
    assert written - set(cfg) <= {"input_scale", "output_scale"}
    assert set(cfg) - written == ({"seed"} & set(cfg)) | ({"rebase"} if name == "batch_tiny" else set())
    assert all(_plain(d["run_args"][key]) == _plain(cfg[key]) for key in ("logrows", "num_inner_cols", "decomp_base", "decomp_legs"))
    assert all(d[key] == _plain(cfg[key]) for key in set(d) - {"model", "run_args", "output_scale"} if key in cfg)
    path = tmp_path / "c.json"
    path.write_text(json.dumps(d))
    loaded, _ = X._load_circuit(str(path))
    assert type(loaded) is type(c) and _same(loaded.config(), cfg) and loaded.plan_identity() == c.plan_identity()
    for other in ("mlp", "scatter_gather", "sort_topk", "sum_prod"):
        with pytest.raises(ValueError, match="no JSON description for a %s" % type(CASES[other][0]()).__name__):
            X.describe(CASES[other][0]())


def _hash(prefix, circuit, tables=True):
    """sha256 of the prefix, the identity and, per static lookup table in the order of their names, the name, (lo, hi, col_size) as three
    little-endian int64 and the table's values over [lo, hi] as int64"""
    h = hashlib.sha256(prefix + circuit.plan_identity())
    for table_name, table in sorted(circuit.gc.base.static_tables.items()) if tables else ():
        lo, hi = table.range
        h.update(table_name.encode() + struct.pack("<3q", lo, hi, table.col_size) + np.array([table.f(x) for x in range(lo, hi + 1)], np.int64).tobytes())
    return h.digest()


@pytest.mark.parametrize("name", [name for name in CASES if name != "sum_prod"])
def test_params_hash_is_the_documented_prefix_the_identity_and_the_tables(name):
    from ezkl_amd import witness_plan as WP
    c = CASES[name][0]()
    prefix = b"" if name == "mlp" else ("layout:%s:" % type(c).__name__).encode()
    assert WP.params_hash(c) == _hash(prefix, c)
    assert (len(c.gc.base.static_tables) > 0) == (name in ("conv_k6", "norm_softmax", "attention"))       # (the cases cover both)


def test_params_hash_of_the_standalone_einsums_and_the_surrogate():
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    matmul, general = EL.EinsumMatmulCircuit(8, 2), EL.EinsumCircuit(8, "ij,jk->ik", dict(i=2, j=3, k=2))
    assert WP.params_hash(matmul) == _hash(b"phased:", matmul, tables=False)
    assert WP.params_hash(general) == _hash(b"einsum:", general, tables=False)                  # (the subclass has a prefix of its own)
    surrogate = EL.TransformerSurrogateCircuit(10, blocks=2, d=4, einsum_len=3, decomp_base=16, lookup_max=64)
    assert WP.params_hash(surrogate) == _hash(b"layout:TransformerSurrogateCircuit:", surrogate) and len(surrogate.gc.base.static_tables) == 3


def test_second_phase_advice_that_is_not_declared_is_refused():
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP

    class Undeclared(EL.AttentionHeadCircuit):
        lays_einsums = False

    c = Undeclared(10, 4, 4, 2, capacity=6 << 10)
    assert any(col.phase != 0 for col in c.gc.cs.advice) and callable(c.layout)
    with pytest.raises(WP.PlanError, match="witness plans do not cover second-phase advice"):
        WP.record_plan(c)
    assert WP.record_plan(BF.attention()).n_phases == 2
