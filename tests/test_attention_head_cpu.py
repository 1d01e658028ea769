"""One attention head whose matmuls are Freivalds einsums over tensors the circuit computed (ezkl_layout.AttentionHeadCircuit), without a
GPU: at n = 4 tokens, e = 4, d = 2 the oracle MockProver accepts the layout with both phases, the recorded two-phase plan replays to the
layout's columns and outputs, and from the second einsum on the claimed products read CELLS -- the products of the einsums before them
-- not model inputs: an einsum can follow another op."""
import numpy as np
import pytest

K, N, E, D = 10, 4, 4, 2
CHAL = [0x1234567890abcdef1234567890abcdef, 0xfedcba0987654321]
_BUILT = {}


def circuit():
    from ezkl_amd import ezkl_layout as EL
    return EL.AttentionHeadCircuit(K, N, E, D, capacity=6 << K)


def built():
    """(circuit, build(as_ints), the recorded plan): made once, shared, never modified"""
    from ezkl_amd import witness_plan as WP
    if not _BUILT:
        c = circuit()
        _BUILT.update(c=c, b=c.build(as_ints=True), plan=WP.record_plan(circuit()).validate())
    return _BUILT["c"], _BUILT["b"], _BUILT["plan"]


def columns(b, chal):
    cols = {**b["advice"](0, []), **b["advice"](1, chal)}
    return [cols[i] for i in range(b["cs"].n_advice)]


def test_the_settings_come_from_the_five_analyses():
    from ezkl_amd import einsum_plan as EP
    c, b, _ = built()
    per = [EP.einsum_analysis(eq, dims).reduction_length for eq, dims in c.equations]
    assert [eq for eq, _ in c.equations] == ["ie,ed->id"] * 3 + ["id,jd->ij", "ij,jd->id"]
    assert c.settings.einsum_reduction_length == sum(per) and c.settings.einsum_max_output_axes == 2
    assert b["cs"].n_challenges == 2 and sorted(set(b["cs"].advice_phase)) == [0, 1]


def test_mock_prover_accepts_the_head_and_rejects_a_wrong_score():
    from ezkl_amd import ezkl_layout as EL
    from oracle import mock_prover as MP
    R = EL.R
    c, b, _ = built()
    cs, chal = b["cs"], [v % R for v in CHAL]
    adv = columns(b, chal)
    assert MP.check(cs, adv, b["fixed"], b["instances"], b["copies"], challenges=chal) == []
    # the model, on integers: the instance is round(softmax-weighted V) as the circuit's rebase divisions round it
    x = np.array(c.default_inputs()).reshape(N, E)
    Q, Kt, V = x @ c.Wq, x @ c.Wk, x @ c.Wv
    S = np.vectorize(lambda s: EL.round_div(int(s), c.score_div))(Q @ Kt.T)
    ex = np.vectorize(c.exp)(S - S.max(1, keepdims=True))
    inv = [EL.recip_claim(int(t), c.input_scale * c.output_scale, 0) for t in ex.sum(1)]
    O = (ex * np.array(inv)[:, None]) @ V
    assert b["instances"] == [[EL.round_div(int(v), c.out_div) % R for v in O.reshape(-1)]]
    # a wrong entry of the scores' claimed product (the fourth einsum: its cells follow the three projections' in the einsum columns)
    first_rows = sum(ein.reduction_length + 2 for ein in c.eins[:3])
    ein_col = cs.n_advice - 6                                          # the Freivalds columns are configured last: first-phase RLC input
    assert adv[ein_col][first_rows] == int((Q @ Kt.T)[0, 0]) % R
    bad = [list(col) for col in adv]
    bad[ein_col][first_rows] = (bad[ein_col][first_rows] + 1) % R
    assert MP.check(cs, bad, b["fixed"], b["instances"], b["copies"], challenges=chal)


def test_the_plan_equals_the_layout_and_later_einsums_read_cells():
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    R = EL.R
    c, b, plan = built()
    cs, chal = b["cs"], [v % R for v in CHAL]
    adv = columns(b, chal)
    assert (plan.n_phases, plan.n_challenges, plan.n_inputs, len(plan.outputs)) == (2, 2, N * E, N * D)
    assert WP.column_phases(plan) == cs.advice_phase and plan.param_hash == WP.params_hash(c)
    cols, outs = WP.run_plan_host(plan, c.default_inputs(), challenges=chal)
    for i in range(cs.n_advice):
        assert cols[i] == adv[i], "advice column %d differs" % i
    assert [outs] == b["instances"]
    kinds = plan.records[:, 0].tolist()
    assert WP.MATMUL not in kinds and all(kd not in WP.UNASSIGNED_KINDS and kd < WP.KINDS_TOP for kd in kinds)
    # the five claims, in order: one-step DOT records in phase 0 of |O| dots of K products
    recs = plan.records.tolist()
    claims = [(ri, r) for ri, r in enumerate(recs) if r[0] == WP.DOT and r[7] == 0 and r[3] == 1 and r[2] in (E, D, N)
              and r[1] in (N * D, N * N)]
    assert [r[1:4] for _, r in claims] == [[N * D, E, 1]] * 3 + [[N * N, D, 1], [N * D, N, 1]]
    writer = {}                                                        # cell -> the record that writes it
    for ri, (kind, count, p0, p1, dst, a_, b_, phase) in enumerate(recs):
        for cell in plan.pool[dst:dst + WP.dst_words(kind, count, p1)].tolist():
            if cell != WP.NONE:
                writer[cell] = ri
    model_cols = set(v.inner[x_][y].index for v in c.gc.advices[:3] for x_ in range(v.num_blocks()) for y in range(v.num_inner_cols))
    def sources(r, which):
        cells = plan.pool[r[which]:r[which] + r[1] * r[2]].tolist()
        return cells, set(recs[writer[cell]][0] for cell in cells)
    for at, (ri, r) in enumerate(claims):
        (cells_a, kinds_a), (cells_b, kinds_b) = sources(r, 5), sources(r, 6)
        assert all(writer[cell] < ri for cell in cells_a + cells_b), "a claim reads cells of earlier records only"
        if at < 3:                                                     # X: placed model cells; W: parameters placed by the einsum itself
            assert kinds_a == {WP.INPUT} and kinds_b == {WP.PARAM} and set(cell >> K for cell in cells_a) <= model_cols
    score, out = claims[3][1], claims[4][1]
    claimed = [set(plan.pool[r[4]:r[4] + r[1]].tolist()) for _, r in claims]
    assert set(sources(score, 5)[0]) == claimed[0] and set(sources(score, 6)[0]) == claimed[1], "Q . K^T reads the cells the projections claimed"
    assert set(sources(out, 6)[0]) == claimed[2] and sources(out, 5)[1] == {WP.MUL} and set(cell >> K for cell in sources(out, 5)[0]) <= model_cols
    # other inputs: the same plan
    x2 = np.random.default_rng(9).integers(-4, 5, N * E).tolist()
    other = circuit().build(as_ints=True, inputs=x2)
    cols2, outs2 = WP.run_plan_host(plan, x2, challenges=chal)
    assert cols2 == columns(other, chal) and [outs2] == other["instances"]


def test_recording_an_einsum_over_cells_no_longer_needs_model_inputs():
    """before the general einsum a recording region refused every einsum whose operands were not model inputs"""
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    from test_witness_plan_ops_cpu import _surrogate
    _, _, plan = built()
    assert plan.n_records < 400 and plan.n_ops > 5
    s = _surrogate(10)
    reg, cell = WP.PhasedLookupRecordingRegion(s.gc), EL.Val(WP._Cell(0))
    with pytest.raises(WP.PlanError, match="not model inputs"):         # the hard-wired matmul layout keeps its rule
        reg.einsum(s.ein, [[cell] * s.L] * s.L, [[cell] * s.L] * s.L)
