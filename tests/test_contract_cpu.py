"""CONTRACT records and the version-2 blob without a GPU: both validators (the C++ one as tests/cpp/test_witness_plan_contract.cpp under the
sanitizers), the host interpreter against a direct Python-integer contraction, and circuits recorded with einsum_claim="contract"."""
import hashlib
import json

import numpy as np
import pytest

import batch_mlp_cases as F
import wplan_cpp

K, M31 = 12, (1 << 31) - 1
SHAPES = [(1, 1, 1), (1, 17, 1), (63, 15, 65), (64, 16, 64), (65, 33, 63), (129, 17, 3), (3, 257, 130)]
PATTERNS = ["max", "alternating", "zeros", "repeated"]
BATCHED = ("bij,bjk->bik", dict(b=2, i=3, j=4, k=2))
# per circuit: sha256 of the default recording's blob on the commit before the claim form existed; (count, kd, n) of its CONTRACT records
CIRCUITS = {"attention": ("c6e73a833525d111f40407d88b9fb6dd82a63c5051fa21a4e8677f885b988782", [(8, 4, 2)] * 3 + [(16, 2, 4), (8, 4, 2)]),
            "bij,bjk->bik": ("469bc166ed884086e8cb45d42e57cf51bfe142ce11e28ce1615495990da056e8", [(6, 4, 2)] * 2),
            "mlp_batch": ("4bbf826a7d2d668d17ce957abf510e1b621ec717fe6dd9a27f9c217b25036c5a", [(4, 2, 2)])}


def operands(m, kd, n, pattern, seed=0):
    """(A, B) flat and row-major: all 2^31 - 1 (the sum passes 2^64 from kd = 5), B's rows -(2^31 - 1) and 2^31 - 2 in turn, zeros, seeded"""
    if pattern == "repeated":
        return [np.random.default_rng(seed).integers(-M31, M31 + 1, size).tolist() for size in (m * kd, kd * n)]
    b = {"max": lambda t: M31, "alternating": lambda t: M31 - 1 if t % 2 else -M31, "zeros": lambda t: 0}[pattern]
    return [0 if pattern == "zeros" else M31] * (m * kd), [b(t) for t in range(kd) for _ in range(n)]


def contract_plan(shapes, repeated=False, phase=0, k=K):
    """every shape's operands as inputs placed by one INPUT record, then one CONTRACT record per shape, its destinations from a fresh column
    on; repeated: row 0 of a names ONE cell.  -> (plan, per record: (the inputs a names, those b names, the destination cells))"""
    from ezkl_amd import witness_plan as WP
    n_in = sum(m * kd + kd * n for m, kd, n in shapes)
    at, cell, pool, records, layout = 0, -(-n_in // (1 << k)) << k, list(range(n_in)) * 2, [[WP.INPUT, n_in, 0, 0, 0, n_in, 0, 0]], []
    for m, kd, n in shapes:
        a, b, dst = list(range(at, at + m * kd)), list(range(at + m * kd, at + m * kd + kd * n)), list(range(cell, cell + m * n))
        if repeated:
            a[:kd] = [a[0]] * kd
        records.append([WP.CONTRACT, m * n, kd, n, len(pool), len(pool) + m * n, len(pool) + m * n + m * kd, phase])
        pool += dst + a + b
        layout.append((a, b, dst))
        at, cell = at + m * kd + kd * n, cell + m * n
    return WP.WitnessPlan(k, -(-cell // (1 << k)), n_in, [], [], records, [], pool, n_in + sum(m * n for m, _, n in shapes), len(records), b"\0" * 32,
                          n_phases=phase + 1), layout


def expected_columns(plan, layout, shapes, x):
    """the columns after the run, by a direct contraction over Python integers reduced mod r: nothing of the plan is interpreted"""
    from ezkl_amd import ezkl_layout as EL
    cells = [v % EL.R for v in x] + [0] * ((plan.n_advice << plan.k) - len(x))
    for (m, kd, n), (a, b, dst) in zip(shapes, layout):
        for i in range(m):
            for j in range(n):
                cells[dst[i * n + j]] = sum(x[a[i * kd + t]] * x[b[t * n + j]] for t in range(kd)) % EL.R
    return [cells[c << plan.k:(c + 1) << plan.k] for c in range(plan.n_advice)]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_the_host_interpreter_equals_a_direct_contraction(pattern):
    from ezkl_amd import witness_plan as WP
    shapes = [(1, 17, 1), (5, 3, 7)]
    plan, layout = contract_plan(shapes, repeated=pattern == "repeated")
    assert plan.validate().version == 2 and WP.WitnessPlan.from_bytes(plan.to_bytes()).validate() == plan
    x = sum((v for s in shapes for v in operands(*s, pattern)), [])
    assert WP.run_plan_host(plan, x)[0] == expected_columns(plan, layout, shapes, x)


@pytest.mark.parametrize("at,value", [(7, 1 << 31), (7, -(1 << 31)), (3 * 5 + 11, 1 << 31), (3 * 5 + 11, -(1 << 31))])
def test_the_reported_element_in_a_and_in_b(at, value):
    from ezkl_amd import witness_plan as WP
    plan, _ = contract_plan([(3, 5, 4)])
    x = sum(operands(3, 5, 4, "max"), [])
    x[at], x[-1] = value, 1 << 40                                   # the smallest failing element is the one reported
    with pytest.raises(AssertionError, match=r"einsum operand outside the exact-product range \(contract record 1, element %d\)" % at):
        WP.run_plan_host(plan, x)


def _edited(words, field, value):
    plan, _ = contract_plan([(3, 5, 4)])
    plan.records[1, field] = plan.records[1, 4] if value is None else value      # None: the offset of the record's own destinations
    return words, 1, plan


def test_both_validators_take_version_2_refuse_its_defects_and_kind_32_in_version_1(tmp_path):
    """the C++ parser as a plain program under the sanitizers: the good blobs, each again under a version-1 header, and every shape
    defect (kd = 0, n = 0, count % n != 0, b past the pool, a past the pool) with the words `validate` refuses it with"""
    from ezkl_amd import witness_plan as WP
    good = [contract_plan([(3, 5, 4)])[0], contract_plan([(65, 33, 63), (1, 17, 1)], repeated=True, phase=1)[0]]
    bad = [_edited("bad contract shape", field, value) for field, value in ((2, 0), (3, 0), (3, 5), (6, 1 << 30), (2, 1 << 31))]
    wplan_cpp.parser_program(tmp_path, "test_witness_plan_contract", good, bad + [_edited("a cell is read before an earlier record has written it", 5, None)])
    blob = bytearray(good[0].to_bytes())
    blob[4] = 1
    with pytest.raises(WP.PlanError, match="record 1: unknown kind 32"):
        WP.WitnessPlan.from_bytes(bytes(blob)).validate()


def recorded(name, **kw):
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    c = (EL.AttentionHeadCircuit(10, 4, 4, 2, capacity=6 << 10, **kw) if name == "attention" else
         EL.BatchMlpCircuit(9, 1, 2, F.TINY["weights"], F.TINY["biases"], F.BASE, F.LEGS, **kw) if name == "mlp_batch" else EL.EinsumCircuit(8, *BATCHED, **kw))
    return c, WP.record_plan(c).validate()


@pytest.mark.parametrize("name", list(CIRCUITS))
def test_recorded_with_the_contract_claim(tmp_path, name):
    from ezkl_amd import ezkl_layout as EL, execute as X, witness_plan as WP
    (c, plan), (_, dot), told_nothing = recorded(name, einsum_claim="contract"), recorded(name, einsum_claim="dot"), recorded(name)[1].to_bytes()
    assert dot.to_bytes() == told_nothing and dot.version == 1 and hashlib.sha256(told_nothing).hexdigest() == CIRCUITS[name][0]
    claims = [tuple(r[1:4]) for r in plan.records.tolist() if r[0] == WP.CONTRACT and r[7] == 0]
    assert plan.version == 2 and claims == CIRCUITS[name][1] and plan.param_hash == WP.params_hash(c) != dot.param_hash
    chal = [0x1234567890abcdef1234567890abcdef % EL.R, 0xfedcba0987654321, 77][:plan.n_challenges]
    if name == "bij,bjk->bik":
        x = np.random.default_rng(3).integers(-9, 10, c.n_inputs).tolist()
        fn = c.advice_fn(x[:c.sizes[0]], x[c.sizes[0]:], 6)
    else:
        x, fn = c.default_inputs(), c.build(as_ints=True)["advice"]
        (tmp_path / "c.json").write_text(json.dumps(X.describe(c)))     # the description states the claim form, and only when it is not the default
        assert X._load_circuit(str(tmp_path / "c.json"))[0].plan_identity() == c.plan_identity() and "einsum_claim" not in X.describe(recorded(name)[0])
    layout = {**fn(0, []), **fn(1, chal)}
    for phase in (0, None):                                          # phase 0 alone, then both: the layout's cells, and the "dot" plan's
        cols = WP.run_plan_host(plan, x, challenges=chal, phase=phase)
        assert cols == WP.run_plan_host(dot, x, challenges=chal, phase=phase)
        assert all(col == [v % EL.R for v in layout[i]] for i, col in enumerate(cols[0]) if phase is None or WP.column_phases(plan)[i] == 0)
