"""Batched MLPs and the attention head at the file level, without a GPU (ezkl_layout.BatchMlpCircuit, execute.FAMILIES "mlp_batch" and
"attention"): a description round-trips to its circuit; `gen_witness` on the host gives, row by row, what the existing batch-1 family
computes; the recorded plan has two phases and replays to the layout's columns; the oracle MockProver accepts both phases and names a
second-phase gate when a claimed product is off by one; what the layout does not cover is refused by name."""
import json

import pytest

import batch_mlp_cases as F

NAMES = list(F.BATCH_CASES)
_BUILT = {}


def built(name):
    """(circuit, build(as_ints) on the case's first input, the recorded plan): made once, shared, never modified"""
    from ezkl_amd import witness_plan as WP
    if name not in _BUILT:
        make = F.attention if name == "attention" else lambda: F.batch(F.BATCH_CASES[name][0])
        c = make()
        x = c.default_inputs() if name == "attention" else F.BATCH_CASES[name][1][0]
        _BUILT[name] = (c, c.build(as_ints=True, inputs=x), WP.record_plan(make()).validate(), x)
    return _BUILT[name]


def _signed_outputs(w):
    from ezkl_amd import ezkl_layout as EL
    return [EL.signed(int.from_bytes(bytes.fromhex(o), "little")) for o in w["outputs"][0]]


def _write(tmp_path, j, name="c.json"):
    path = str(tmp_path / name)
    open(path, "w").write(json.dumps(j))
    return path


@pytest.mark.parametrize("name", NAMES + ["attention"])
def test_a_description_round_trips_to_the_circuit_it_describes(tmp_path, name):
    """(on the parent commit: unsupported compiled circuit: 'mlp_batch')"""
    from ezkl_amd import execute as X, witness_plan as WP
    direct = built(name)[0]
    j = X.describe(direct)
    assert j["model"] == ("attention" if name == "attention" else "mlp_batch")
    loaded, parsed = X._load_circuit(_write(tmp_path, j))
    assert type(loaded) is type(direct) and parsed == json.loads(json.dumps(j))
    assert loaded.plan_identity() == direct.plan_identity() and WP.params_hash(loaded) == WP.params_hash(direct)
    assert loaded.n_inputs == direct.n_inputs and len(loaded.gc.cs.advice) == len(direct.gc.cs.advice)
    assert loaded.settings.model_instance_shapes == direct.settings.model_instance_shapes
    fresh = loaded.fresh()
    assert fresh.gc.cs is not loaded.gc.cs and fresh.plan_identity() == direct.plan_identity() and X.describe(fresh) == j
    assert X._phased(loaded) and sorted(set(c.phase for c in loaded.gc.cs.advice)) == [0, 1]


def test_the_settings_come_from_the_analyses_and_the_blocks_are_the_cases():
    from ezkl_amd import einsum_plan as EP
    for name in NAMES:
        c, b, _, _ = built(name)
        per = [EP.einsum_analysis(eq, dims) for eq, dims in c.equations]
        assert all(eq == "mk,nk->mn" and a.strategy == EP.FREIVALDS for (eq, _), a in zip(c.equations, per))
        assert c.settings.einsum_reduction_length == sum(a.reduction_length for a in per) and c.settings.einsum_max_output_axes == 2
        assert c.settings.model_instance_shapes == [[c.m, c.n_out]] and c.n_inputs == c.m * c.n_in
        assert b["cs"].n_challenges == 2 and sorted(set(b["cs"].advice_phase)) == [0, 1]
        assert all(v.num_blocks() == 1 for v in c.gc.base.einsums.inputs + c.gc.base.einsums.outputs)
    assert built("tiny")[0].gc.advices[0].num_blocks() == 1 and built("ragged")[0].gc.advices[0].num_blocks() == 3
    two = built("two_blocks")[0]
    assert two.gc.advices[0].num_blocks() == 2 and two.synthesize(F.BATCH_CASES["two_blocks"][1][0]).linear > two.gc.advices[0].block_size()


@pytest.mark.parametrize("name", NAMES)
def test_every_row_of_the_batch_is_the_batch_one_family_s_forward_pass(tmp_path, name):
    """the oracle is the existing "mlp" family: _forward_mlp on a batch-1 description with the same weights and rebase, row by row"""
    from ezkl_amd import execute as X
    spec, xs = F.BATCH_CASES[name]
    m, k = spec["batch"], len(spec["weights"][0][0])
    compiled = _write(tmp_path, X.describe(built(name)[0]))
    one = dict(X.FAMILIES["mlp"].describe(F.describe_as_mlp(spec)), family="mlp")
    for x in xs:
        w = X.gen_witness(compiled, F.data(x))
        rows = [X._forward_mlp(one, x[i * k:(i + 1) * k])[0] for i in range(m)]
        assert _signed_outputs(w) == [v for row in rows for v in row]
        assert (w["min_lookup_inputs"], w["max_lookup_inputs"], w["max_range_size"]) == (0, 0, F.BASE - 1)
    assert any(abs(v) == F.BOUND - 1 for v in xs[-1]), "the last input of a case sits at the decomposition bound minus one"
    for sign in (1, -1):                                                # one past it: the MLP family's ValueError
        past = list(xs[0])
        past[-1] = sign * F.BOUND
        with pytest.raises(ValueError, match="exceeds the decomposition range") as batch_error:
            X.gen_witness(compiled, F.data(past))
        with pytest.raises(ValueError, match="exceeds the decomposition range") as one_error:
            X._forward_mlp(one, past[-k:])
        assert type(batch_error.value) is type(one_error.value) is ValueError


def _columns(b, chal):
    cols = {**b["advice"](0, []), **b["advice"](1, chal)}
    return [cols[i] for i in range(b["cs"].n_advice)]


@pytest.mark.parametrize("name", NAMES)
def test_the_plan_has_two_phases_and_replays_to_the_layout_phase_by_phase(name):
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    c, b, plan, x = built(name)
    cs, chal = b["cs"], [v % EL.R for v in F.CHAL]
    adv = _columns(b, chal)
    assert (plan.n_phases, plan.n_challenges, plan.n_inputs, len(plan.outputs)) == (2, 2, c.n_inputs, c.m * c.n_out)
    assert WP.column_phases(plan) == cs.advice_phase and plan.param_hash == WP.params_hash(c)
    first, outs0 = WP.run_plan_host(plan, x, phase=0)
    both, outs = WP.run_plan_host(plan, x, challenges=chal)
    for i in range(cs.n_advice):
        assert both[i] == adv[i], "advice column %d differs" % i
        if cs.advice_phase[i] == 0:
            assert first[i] == adv[i], "phase 0 alone: advice column %d differs" % i
    assert outs == c.outputs == b["instances"][0]
    kinds = plan.records[:, 0].tolist()
    assert WP.MATMUL not in kinds and all(kd not in WP.UNASSIGNED_KINDS and kd < WP.KINDS_TOP for kd in kinds) and WP.VERSION == 1
    # every layer's claimed product: one one-step DOT record over cells, in phase 0
    recs = plan.records.tolist()
    ein_col = c.gc.base.einsums.inputs[0].inner[0][0].index
    lands_in = lambda r: set(cell >> c.k for cell in plan.pool[r[4]:r[4] + WP.dst_words(r[0], r[1], r[3])].tolist())
    claims = [r[1:4] for r in recs if r[0] == WP.DOT and r[7] == 0 and lands_in(r) == {ein_col}]
    assert claims == [[c.m * len(W), len(W[0]), 1] for W in c.weights]
    assert all(r[3] == F.LEGS and r[2] == 1 for r in recs if r[0] == WP.DOT and r[7] == 0 and lands_in(r) != {ein_col}), "every other: a recomposition"
    # other inputs: the same plan
    for x2 in F.BATCH_CASES[name][1][1:]:
        other = F.batch(F.BATCH_CASES[name][0]).build(as_ints=True, inputs=x2)
        cols2, outs2 = WP.run_plan_host(plan, x2, challenges=chal)
        assert cols2 == _columns(other, chal) and [outs2] == other["instances"]


def _second_phase_gates(cs):
    """the gates that read a second-phase advice column or a challenge"""
    def late(e, seen):
        if id(e) in seen:
            return seen[id(e)]
        op = e.node[0]
        r = op == "chal" or (op == "adv" and cs.advice_phase[e.node[1]] > 0) or \
            (op not in ("const", "chal", "adv", "fix", "inst") and any(late(x, seen) for x in e.node[1:] if hasattr(x, "node")))
        seen[id(e)] = r
        return r
    seen = {}
    return {gi for gi, g in enumerate(cs.gates) if late(g, seen)}


@pytest.mark.parametrize("name", NAMES)
def test_the_mock_prover_accepts_both_phases_and_a_wrong_product_fails_a_second_phase_gate(name):
    from ezkl_amd import ezkl_layout as EL
    from oracle import mock_prover as MP
    R = EL.R
    c, b, _, x = built(name)
    cs, chal = b["cs"], [v % R for v in F.CHAL]
    adv = _columns(b, chal)
    assert MP.check(cs, adv, b["fixed"], b["instances"], b["copies"], challenges=chal) == []
    # the first layer's claimed product: the first cells of the first-phase RLC input column (the Freivalds columns are configured last)
    ein_col = cs.n_advice - 6
    k = c.n_in
    relu = (lambda v: max(v, 0)) if c.relu_first else (lambda v: v)
    want = sum(relu(a) * w for a, w in zip(x[:k], c.weights[0][0]))
    assert EL.signed(adv[ein_col][0]) == want
    bad = [list(col) for col in adv]
    bad[ein_col][0] = (bad[ein_col][0] + 1) % R
    fails = MP.check(cs, bad, b["fixed"], b["instances"], b["copies"], challenges=chal, max_failures=64)
    failed_gates = {int(f.split()[1]) for f in fails if f.startswith("gate")}
    assert failed_gates & _second_phase_gates(cs), "a claimed product off by one fails a second-phase gate: %r" % fails


def test_what_the_layout_does_not_cover_is_refused_by_name(tmp_path):
    from ezkl_amd import execute as X, ezkl_layout as EL
    good = X.describe(built("ragged")[0])
    def refused(match, **fields):
        j = json.loads(json.dumps(good))
        for key, v in fields.items():
            at, path = j, key.split("__")
            for p in path[:-1]:
                at = at[p]
            if v is None:
                del at[path[-1]]
            else:
                at[path[-1]] = v
        with pytest.raises(ValueError, match=match):
            X._load_circuit(_write(tmp_path, j))
    base_ops = "lays out with base ops"
    refused(base_ops + ".*batch 1 is MlpCircuit's", batch=1)
    with pytest.raises(ValueError, match=base_ops):                             # a layer with n = 1
        EL.BatchMlpCircuit(9, 1, 2, [[[1, 2]]], [[1]], F.BASE, F.LEGS)
    refused(r"layer 1 \(m = 3, k = 4, n = 1\).*" + base_ops, weights=good["weights"][:1] + [[[1, -1, 2, 0]]], biases=[good["biases"][0], [3]])
    with pytest.raises(ValueError, match=r"k = 1.*" + base_ops):                # k = 1: the sanitised equation has no common index
        EL.BatchMlpCircuit(9, 1, 2, [[[1], [2]]], [[1, 2]], F.BASE, F.LEGS)
    refused(r"k = 1, n = 2.*" + base_ops, weights=[[[1], [2]]], biases=[[1, 2]], rebase=[4])
    # the ragged shape with two inner columns: the einsum layout places one entry a row, and a witness plan's RLC record states one
    refused(r'"run_args.num_inner_cols" must be 1 in the "mlp_batch" family', run_args__num_inner_cols=2)
    with pytest.raises(ValueError, match="num_inner_cols = 2: " + EL.EINSUM_WIDTH_ERROR):
        F.batch(F.RAGGED, num_inner_cols=2)
    for key, v, match in (("batch", 0, '"batch"'), ("batch", "3", '"batch"'), ("batch", None, '"batch" is missing'), ("batch", True, '"batch"'),
                          ("weights", None, '"weights" is missing'), ("weights", [], '"weights"'), ("weights", [[[1.5, 2, 3, 0, 1]]], '"weights"'),
                          ("weights", [[1, 2]], '"weights"'), ("biases", None, '"biases" is missing'), ("biases", [[1, "2", 0, 2], [3, -4]], '"biases"'),
                          ("biases", [[1, -1, 0, 2]], '"biases" takes one vector per matrix'), ("biases", [[1, -1, 0], [3, -4]], "layer 0"),
                          ("weights", [good["weights"][0], [[1, -1, 2], [0, 3, -2]]], "layer 1"),
                          ("rebase", [4], '"rebase"'), ("rebase", [4, 0], '"rebase"'), ("rebase", "4", '"rebase"'), ("rebase", [4, 1 << 32], '"rebase"'),
                          ("output_scale", "0", '"output_scale"'), ("output_scale", None, '"output_scale" is required'), ("relu_last", 1, '"relu_last"'),
                          ("relu_first", "no", '"relu_first"'), ("capacity", 0, '"capacity"'), ("capacity", 2.5, '"capacity"'),
                          ("run_args", None, '"run_args"'), ("run_args__logrows", None, '"run_args.logrows" is missing'),
                          ("run_args__decomp_base", 1, '"run_args.decomp_base"'), ("run_args__decomp_legs", "2", '"run_args.decomp_legs"'),
                          ("run_args__input_scale", 1.5, '"run_args.input_scale"'),
                          ("run_args__input_visibility", "Public", "unsupported visibility: input is Public"),
                          ("run_args__param_visibility", "Fixed", "unsupported visibility: params is Fixed"),
                          ("run_args__output_visibility", {"Hashed": {}}, "unsupported visibility: output is Hashed")):
        refused(match, **{key: v})
    head = X.describe(built("attention")[0])
    for key, v, match in (("n", 0, '"n"'), ("e", None, '"e" is missing'), ("d", "2", '"d"'), ("capacity", None, '"capacity"'), ("input_scale", 0, '"input_scale"'),
                          ("output_scale", -1, '"output_scale"'), ("eps", 0, '"eps"'), ("score_div", 0, '"score_div"'), ("lookup_range", [0, -255], '"lookup_range"'),
                          ("Wq", None, '"Wq" is missing'), ("Wk", [[1, 2]], "Wk: the circuit takes an array of shape"), ("Wv", [[0.5, 1]] * 4, "Wv: every entry is an integer"),
                          ("run_args__num_inner_cols", 2, '"run_args.num_inner_cols" must be 1 in the "attention" family'),
                          ("run_args__output_visibility", "Private", "unsupported visibility: output is Private")):
        j = json.loads(json.dumps(head))
        at, path = j, key.split("__")
        for p in path[:-1]:
            at = at[p]
        if v is None:
            del at[path[-1]]
        else:
            at[path[-1]] = v
        with pytest.raises(ValueError, match=match):
            X._load_circuit(_write(tmp_path, j))
    for model in ("einsum", "surrogate", "sort_topk"):
        with pytest.raises(ValueError) as e:
            X._load_circuit(_write(tmp_path, dict(good, model=model)))
        assert str(e.value) == "unsupported compiled circuit: %r" % model


def test_the_attention_description_carries_its_weights_and_gen_witness_is_the_layout(tmp_path):
    from ezkl_amd import execute as X, ezkl_layout as EL
    c, b, _, x = built("attention")
    j = X.describe(c)
    assert [j[name] for name in ("Wq", "Wk", "Wv")] == [c.Wq.tolist(), c.Wk.tolist(), c.Wv.tolist()]
    w = X.gen_witness(_write(tmp_path, j), F.data(x))
    assert [v % EL.R for v in _signed_outputs(w)] == b["instances"][0]
    assert w["min_lookup_inputs"] < 0 and w["max_lookup_inputs"] == 0       # the exp table's inputs: x - max(row)
    j["Wq"] = (c.Wq + 1).tolist()                                            # given weights, not the seeded ones
    other, _ = X._load_circuit(_write(tmp_path, j, "other.json"))
    assert (other.Wq == c.Wq + 1).all() and (other.fresh().Wq == c.Wq + 1).all() and other.plan_identity() != c.plan_identity()
    assert EL.AttentionHeadCircuit(10, 4, 4, 2, capacity=6 << 10).plan_identity() == c.plan_identity()


def test_the_mlp_family_keeps_its_blobs():
    """batch 1 stays MlpCircuit's, recorder and hash included"""
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    spec = F.TINY
    one = EL.MlpCircuit(spec["logrows"], 1, spec["weights"], spec["biases"], F.BASE, F.LEGS)
    plan = WP.record_plan(one)
    assert plan.n_phases == 1 and not any(c.phase for c in one.gc.cs.advice)
    import hashlib
    assert WP.params_hash(one) == hashlib.sha256(one.plan_identity()).digest()
