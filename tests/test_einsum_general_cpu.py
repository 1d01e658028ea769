"""The general two-operand Freivalds einsum, without a GPU: the planner (ezkl_amd/einsum_plan.py: reduction_planner.rs / analysis.rs
restated), the layout (ezkl_layout.EinsumCircuit: `assign_einsum` for any equation the reference lays out with Freivalds' argument) and its
witness plan (witness_plan.record_plan: the claimed product as ONE DOT record of one step over cells).  For "ij,jk->ik" the general circuit
must lay out what the hard-wired EinsumMatmulCircuit lays out, cell for cell; for every equation the oracle MockProver accepts the layout,
rejects a wrong product element and a changed second-phase cell, the product is numpy's, and the recorded plan replayed by `run_plan_host`
equals `synthesize` column for column in both phases."""
import re

import numpy as np
import pytest

# (equation, dims): rectangular matmul; Q.K^T; a MIXED dot and a second-phase sum; a first-phase sum; BOTH_FIRST products, an RLC with a
# second-phase input and three challenges; a trivial axis
EQUATIONS = [("ij,jk->ik", dict(i=2, j=3, k=4)), ("id,jd->ij", dict(i=3, j=2, d=4)), ("ij,jk->i", dict(i=2, j=3, k=4)),
             ("ij,jk->k", dict(i=2, j=3, k=4)), ("bij,bjk->bik", dict(b=2, i=2, j=3, k=2)), ("aij,jk->aik", dict(a=1, i=2, j=3, k=4))]
IDS = [eq for eq, _ in EQUATIONS]
K = 8
CHAL = [0x1234567890abcdef1234567890abcdef, 0xfedcba0987654321, 0x0f1e2d3c4b5a69788796a5b4c3d2e1f0]
_CASES = {}


def case(eq, dims, seed=1):
    """(circuit, a, b, the plan's input vector): built once, shared, never modified"""
    from ezkl_amd import ezkl_layout as EL
    if (eq, seed) not in _CASES:
        rng = np.random.default_rng(seed)
        a, b = (rng.integers(-128, 128, [dims[c] for c in e]) for e in eq.split("->")[0].split(","))
        _CASES[(eq, seed)] = (EL.EinsumCircuit(K, eq, dims), a, b, [int(v) for v in a.reshape(-1)] + [int(v) for v in b.reshape(-1)])
    return _CASES[(eq, seed)]


def challenges(c):
    from ezkl_amd import ezkl_layout as EL
    return [v % EL.R for v in CHAL[:c.analysis.num_output_axes]]


def host_columns(c, a, b, chal):
    fn = c.advice_fn(a, b, len(c.cs.advice))
    first = fn(0, [])
    return first, {**first, **fn(1, chal)}


def test_the_plan_of_a_matmul_is_the_one_the_bench_circuit_hard_codes():
    from ezkl_amd import einsum_plan as EP
    assert EP.einsum_reductions("ij,jk->ik") == [EP.RLC("ij,i->j", "i", 0, 0, 0), EP.RLC("jk,k->j", "k", 1, 0, 1),
                                                 EP.Contraction("j,j->", "j", [2, 3], [1, 1], 1)]
    for L in (2, 5, 17):
        an = EP.einsum_analysis("ij,jk->ik", dict(i=L, j=L, k=L))
        assert an.reduction_length == 3 * L * L + 2 * L and an.strategy == EP.FREIVALDS
        assert (an.output_indices, an.num_output_axes, an.equation) == (["i", "k"], 2, "ij,jk->ik")
    an = EP.einsum_analysis("aij,jk->aik", dict(a=1, i=2, j=3, k=4))
    assert an.equation == "ij,jk->ik" and an.reduction_length == (2 * 4 + 2) + (2 * 3 + 3 * 4 + 3)
    # the batch axis is in both operands: a pairwise product first, then one RLC per output axis -- the later ones over second-phase tensors
    reds = EP.einsum_reductions("bij,bjk->bik")
    assert reds[0] == EP.Contraction("bij,bjk->bijk", None, [0, 1], [0, 0], 0)
    assert [(r.expression, r.input_phase, r.challenge_index) for r in reds[1:4]] == [("bijk,b->ijk", 0, 0), ("ijk,i->jk", 1, 1), ("jk,k->j", 1, 2)]
    assert reds[4] == EP.Contraction("j->", "j", [5], [1], 1)
    assert EP.einsum_analysis("ij,j->i", dict(i=3, j=4)).strategy == EP.BASE_OPS


@pytest.mark.parametrize("L", [2, 5])
def test_the_general_circuit_lays_out_the_cells_of_the_matmul_circuit(L):
    from ezkl_amd import ezkl_layout as EL
    m, g = EL.EinsumMatmulCircuit(K, L), EL.EinsumCircuit(K, "ij,jk->ik", dict(i=L, j=L, k=L))
    assert g.reduction_length == m.reduction_length and g.n_inputs == m.n_inputs and len(g.cs.advice) == len(m.cs.advice) == 6
    rng = np.random.default_rng(L)
    a, b = rng.integers(-128, 128, (L, L)), rng.integers(-128, 128, (L, L))
    for chal in (None, (CHAL[0] % EL.R, CHAL[1] % EL.R)):               # phase 0, and in full
        r1, r2 = m.synthesize(a, b, chal), g.synthesize(a, b, chal)
        assert r1.advice == r2.advice and r1.fixed == r2.fixed and r1.copies == r2.copies and r1.coord == r2.coord
        rows = lambda reg: [None if x is None else np.nonzero(x)[0].tolist() for x in reg.activations]
        assert rows(r1) == rows(r2)


@pytest.mark.parametrize("eq,dims", EQUATIONS, ids=IDS)
def test_mock_prover_accepts_the_layout_and_rejects_a_wrong_product_and_a_changed_second_phase_cell(eq, dims):
    from ezkl_amd import ezkl_layout as EL
    from oracle import mock_prover as MP
    R = EL.R
    c, a, b, _ = case(eq, dims)
    want = [int(v) % R for v in np.einsum(eq, a, b).reshape(-1)]
    assert [v % R for v in c.einsum(a, b)] == want
    fresh = EL.EinsumCircuit(K, eq, dims)                               # (compress_selectors rewrites a system in place)
    cs, fixed, copies, rows = fresh.keygen_inputs(a, b)
    assert rows == c.reduction_length + 2 <= cs.usable and cs.n_challenges == c.analysis.num_output_axes
    chal = challenges(c)
    _, cols = host_columns(c, a, b, chal)
    adv = [cols[i] for i in range(cs.n_advice)]
    assert adv[0][:len(want)] == want, "the claimed product opens the first-phase RLC input column"
    assert MP.check(cs, adv, fixed, [], copies, challenges=chal) == []
    bad = [list(x) for x in adv]
    bad[0][len(want) - 1] = (bad[0][len(want) - 1] + 1) % R             # one entry of the claimed product
    assert MP.check(cs, bad, fixed, [], copies, challenges=chal)
    second = [i for i in range(cs.n_advice) if cs.advice_phase[i] == 1]
    for col in second:                                                  # one cell of every second-phase column the layout uses
        used = [r for r in range(rows) if adv[col][r]]
        if used:
            bad = [list(x) for x in adv]
            bad[col][used[len(used) // 2]] = (bad[col][used[len(used) // 2]] + 1) % R
            assert MP.check(cs, bad, fixed, [], copies, challenges=chal), "a changed cell of column %d goes unnoticed" % col
    assert any(any(adv[col]) for col in second)


@pytest.mark.parametrize("eq,dims", EQUATIONS, ids=IDS)
def test_the_recorded_plan_replays_to_the_layout_in_both_phases(eq, dims):
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    c, a, b, x = case(eq, dims)
    plan = WP.record_plan(c).validate()
    assert WP.VERSION == 1 and WP.KINDS_TOP == 32
    kinds = plan.records[:, 0].tolist()
    assert all(kd < WP.KINDS_TOP and kd not in WP.UNASSIGNED_KINDS for kd in kinds)
    assert set(kinds) <= {WP.INPUT, WP.COPY, WP.DOT, WP.MUL, WP.RLC, WP.SUMACC, WP.PRODACC} and WP.MATMUL not in kinds
    # the claim: one DOT record in phase 0 of |O| dots of ONE step, K products each, over cells
    n_out = int(np.prod(c.out_shape))
    contracted = int(np.prod([c.dims[ch] for ch in set("".join(c.exprs)) - set(c.analysis.output_indices)]))
    claims = [r for r in plan.records.tolist() if r[0] == WP.DOT and r[7] == 0]
    assert len(claims) == 1 and claims[0][1:4] == [n_out, contracted, 1]
    assert (plan.n_phases, plan.n_challenges, plan.n_inputs, len(plan.outputs)) == (2, c.analysis.num_output_axes, c.n_inputs, 0)
    written = WP.written_columns(plan)                                  # (a column no record writes counts as phase 0)
    assert all(WP.column_phases(plan)[i] == c.cs.advice[i].phase for i in written) and {0, 5} <= set(written)
    assert WP.record_plan(EL.EinsumCircuit(K, eq, dims)).to_bytes() == plan.to_bytes() and plan.param_hash == WP.params_hash(c)
    chal = challenges(c)
    for seed in (1, 5):                                                # the inputs the plan was recorded beside, and others
        _, a2, b2, x2 = case(eq, dims, seed)
        first, both = host_columns(c, a2, b2, chal)
        cols, outs = WP.run_plan_host(plan, x2, phase=0)
        assert outs == [] and all(cols[i] == ref for i, ref in first.items())
        assert all(not any(cols[i]) for i in range(6) if c.cs.advice[i].phase == 1)
        cols, _ = WP.run_plan_host(plan, x2, challenges=chal)
        for i in range(6):
            assert cols[i] == both[i], "advice column %d differs" % i


def test_what_is_out_of_scope_is_refused_by_name_before_anything_is_laid_out():
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    with pytest.raises(ValueError, match=EL.EINSUM_OPERANDS_ERROR):
        EL.EinsumCircuit(K, "bn,anm,bm->ba", dict(a=2, b=2, n=2, m=2))
    with pytest.raises(ValueError, match=EL.EINSUM_OPERANDS_ERROR):
        EL.EinsumCircuit(K, "ij->i", dict(i=2, j=2))
    with pytest.raises(ValueError, match=EL.EINSUM_BASE_OPS_ERROR):
        EL.EinsumCircuit(K, "ij,j->i", dict(i=3, j=4))
    with pytest.raises(ValueError, match=EL.EINSUM_BASE_OPS_ERROR):      # batch 1: one non-common axis is left
        EL.EinsumCircuit(K, "mk,nk->mn", dict(m=1, n=4, k=3))
    with pytest.raises(ValueError, match=EL.EINSUM_REPEAT_ERROR):
        EL.EinsumCircuit(K, "ii,ij->ij", dict(i=2, j=3))
    with pytest.raises(ValueError, match=EL.EINSUM_WIDTH_ERROR):
        EL.EinsumCircuit(K, "ij,jk->ik", dict(i=2, j=3, k=4), num_inner_cols=2)
    with pytest.raises(AssertionError, match="column overflow"):
        EL.EinsumCircuit(5, "ij,jk->ik", dict(i=4, j=4, k=4))
    c = EL.EinsumCircuit.__new__(EL.EinsumCircuit)                       # a claim of 2 * K * |O| > 2^28 words, refused before a layout pass
    c._plan(20, "ij,jk->ik", dict(i=1 << 10, j=1 << 9, k=1 << 10), 1)
    reg = WP.EinsumRecordingRegion(EL.EinsumCircuit(K, "ij,jk->ik", dict(i=2, j=3, k=4)))
    with pytest.raises(WP.PlanError, match=re.escape(WP.CLAIM_ERROR)):
        reg.lay_einsum(c, [[], []])
    assert reg.out.recs == []


def test_the_wide_kernel_takes_no_record_of_an_earlier_family():
    """DOT_WIDE_MIN and the lane rule are the header's, and every DOT record of the plans recorded before this kernel -- whose products per
    step are the circuit's inner columns -- stays below it: the MLP, conv, pool, norm, surrogate and einsum-matmul plans"""
    import os
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    import test_witness_plan_lookup_cpu as TL
    import test_witness_plan_phases_cpu as TP
    from test_witness_plan_cpu import _mlp
    from test_witness_plan_ops_cpu import _surrogate
    hpp = open(os.path.join(os.path.dirname(TL.__file__), "..", "ezkl_amd", "csrc", "witness_plan.hpp")).read()
    m = re.search(r"DOT_WIDE_MIN = (\d+), DOT_WIDE_FILL = 1u << (\d+);", hpp)
    assert (int(m.group(1)), 1 << int(m.group(2))) == (WP.DOT_WIDE_MIN, WP.DOT_WIDE_FILL)
    plans = [WP.record_plan(_mlp(9, 2)[0]), WP.record_plan(TL.CASES["conv_k10_w2"]()[0]), WP.record_plan(EL.PoolClassifierCircuit(10, 2, 12000)),
             WP.record_plan(EL.NormCircuit(10, 2, 12000, 3, 5)), WP.record_plan(_surrogate(10)), TP.recorded(10, 17)[4]]
    widest = max(int(r[2]) for plan in plans for r in plan.records if r[0] == WP.DOT)
    assert widest == 2 < WP.DOT_WIDE_MIN
    # one lane per dot when the dots alone fill the device, more -- a power of two within 64 and p0 -- when there are few long ones
    assert WP.dot_wide_lanes(WP.DOT_WIDE_FILL, 512) == 1 and WP.dot_wide_lanes(1, 512) == 64 and WP.dot_wide_lanes(1, 16) == 16
    assert WP.dot_wide_lanes(1, 17) == 16 and WP.dot_wide_lanes(4096, 512) == 32 and WP.dot_wide_lanes(4096, 16) == 16
    assert WP.dot_wide_lanes(1, 1) == 1 and WP.dot_wide_lanes(1 << 16, 64) == 2
