"""Visibility on files without a GPU: the MLP family with a Public input, Fixed or KZG-committed parameters and a KZG-committed output
(GraphCircuit::configure_with_params / synthesize, src/graph/mod.rs:1945-2200; PolyCommitChip, src/circuit/modules/polycommit.rs).  On all
18 accepted triples the oracle's MockProver accepts the host witness and names the copy or gate a tampered one breaks, the recorded witness
plan replays to the layout's columns, a JSON description and a `model.compiled`-shaped graph load into the same circuit, and what is outside
the family's triples is refused by name.  The default triple stays what it was: same constraint system, same plan blob, same hash."""
import json

import pytest

import visibility_cases as VC

from oracle import mock_prover as MP

N_MODEL_COLUMNS = 18                                             # of the base case under the default triple (asserted below)


def _shape(tri, lengths=(3, 16, 4)):
    """(module columns, instance length) of a triple at the base case, as GraphCircuit::configure_with_params gives them: one unblinded column per committed
    tensor (each fits one), first; the instance column holds the input then the output, each where it is Public"""
    committed = sum(v == "KZGCommit" for v in tri)
    return committed, (lengths[0] if tri[0] == "Public" else 0) + (lengths[2] if tri[2] == "Public" else 0)


def _checked(circuit, x):
    cs, fixed, copies, reg = circuit.keygen_inputs(x)
    adv, inst = circuit.witness(x)
    return cs, fixed, copies, adv, inst, MP.check(cs, adv, fixed, inst, copies)


@pytest.mark.parametrize("tri", VC.TRIPLES, ids=VC.ids)
def test_the_mock_prover_accepts_every_triple_and_the_columns_are_where_the_reference_puts_them(tri):
    from ezkl_amd import ezkl_layout as EL
    circuit = VC.mlp(tri)
    cs, fixed, copies, adv, inst, fails = _checked(circuit, VC.X)
    assert fails == []
    committed, n_inst = _shape(tri)
    cols = circuit.gc.cs.advice
    assert len(cols) == cs.n_advice == N_MODEL_COLUMNS + committed
    assert [c.index for c in cols if not c.blinded] == list(range(committed)) == cs.unblinded
    assert [list(v.inner[0]) for v in circuit.gc.polycommit] == [[cols[i]] for i in range(committed)]
    assert circuit.settings.polycommit_sizes == [n for v, n in zip(tri, (3, 16, 4)) if v == "KZGCommit"]
    assert len(circuit.gc.cs.instance) == 1 and len(inst) == 1 and len(inst[0]) == n_inst
    outs = [29, 0, 19, 17]                                       # relu(W x + b) of the base case
    assert circuit.outputs == outs
    assert inst[0] == ([v % EL.R for v in VC.X] if tri[0] == "Public" else []) + (outs if tri[2] == "Public" else [])
    # the module columns hold the tensors from row 0, in the order input, params, output, and nothing else
    tensors = [t for v, t in zip(tri, (VC.X, circuit.flat_params(), outs)) if v == "KZGCommit"]
    for col, tensor in zip(adv, tensors):
        assert col[:len(tensor)] == [v % EL.R for v in tensor] and not any(col[len(tensor):])
    assert circuit.gc.cs.blinding_factors() == 5


def test_the_default_triple_is_what_it_was():
    """the same constraint system, plan blob and hash as an MlpCircuit that is told nothing about visibility -- and none of the others'"""
    from ezkl_amd import ezkl_layout as EL, plonk as P, witness_plan as WP
    plain = EL.MlpCircuit(VC.K, VC.WIDTH, [VC.WEIGHTS], [VC.BIASES], VC.BASE, VC.LEGS)
    told = VC.mlp(VC.DEFAULT)
    assert len(plain.gc.cs.advice) == N_MODEL_COLUMNS and plain.visibility == VC.DEFAULT and plain.settings.total_const_size == 4
    a, b = plain.keygen_inputs(VC.X), told.keygen_inputs(VC.X)
    assert P.serialize_cs(a[0]) == P.serialize_cs(b[0]) and a[1] == b[1] and a[2] == b[2]
    assert plain.plan_identity() == told.plan_identity() and WP.params_hash(plain) == WP.params_hash(told)
    blob = WP.record_plan(plain).to_bytes()
    assert WP.record_plan(told).to_bytes() == blob
    hashes = {WP.params_hash(VC.mlp(tri)) for tri in VC.TRIPLES}
    assert len(hashes) == 18 and WP.params_hash(plain) in hashes
    assert plain.witness(VC.X) == told.witness(VC.X)


def _named(fails):
    return [f for f in fails if f.startswith("copy (") or f.startswith("gate ")]


def test_a_changed_public_input_fails_a_named_copy():
    from ezkl_amd import ezkl_layout as EL
    for tri in (("Public", "Private", "Public"), ("Public", "Fixed", "KZGCommit")):
        cs, fixed, copies, adv, inst, fails = _checked(VC.mlp(tri), VC.X)
        assert fails == []
        bad = [list(inst[0])]
        bad[0][1] = (bad[0][1] + 1) % EL.R
        fails = MP.check(cs, adv, fixed, bad, copies)
        assert any("inst0,1" in f for f in _named(fails)), fails


def test_a_changed_output_fails_a_named_copy():
    from ezkl_amd import ezkl_layout as EL
    # public output behind a public input: the comparison sits at offset n_inputs of the instance column
    cs, fixed, copies, adv, inst, _ = _checked(VC.mlp(("Public", "Private", "Public")), VC.X)
    bad = [list(inst[0])]
    bad[0][3 + 2] = (bad[0][3 + 2] + 1) % EL.R
    assert any("inst0,5" in f for f in _named(MP.check(cs, adv, fixed, bad, copies)))
    # committed output: the module's cell is tied to the model's output cell
    circuit = VC.mlp(("Private", "Private", "KZGCommit"))
    cs, fixed, copies, adv, inst, _ = _checked(circuit, VC.X)
    bad = [list(a) for a in adv]
    bad[0][2] = (bad[0][2] + 1) % EL.R
    assert any("adv0,2" in f for f in _named(MP.check(cs, bad, fixed, inst, copies)))


@pytest.mark.parametrize("tri", [("KZGCommit", "Private", "Public"), ("Private", "KZGCommit", "Public"), ("KZGCommit", "KZGCommit", "KZGCommit")], ids=VC.ids)
def test_a_changed_module_cell_fails_a_named_copy(tri):
    from ezkl_amd import ezkl_layout as EL
    circuit = VC.mlp(tri)
    cs, fixed, copies, adv, inst, _ = _checked(circuit, VC.X)
    for col, (what, var, length) in enumerate(circuit.committed()):
        for row in (0, length - 1):
            bad = [list(a) for a in adv]
            bad[col][row] = (bad[col][row] + 1) % EL.R
            assert any("adv%d,%d)" % (col, row) in f for f in _named(MP.check(cs, bad, fixed, inst, copies))), (what, row)


def test_a_changed_fixed_parameter_cell_fails_a_named_copy_and_the_parameters_are_in_the_key():
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    circuit = VC.mlp(("Private", "Fixed", "Public"))
    cs, fixed, copies, adv, inst, _ = _checked(circuit, VC.X)
    plan = WP.record_plan(circuit)
    assert len(plan.params) == 0                                  # every parameter is a constant of the plan, as it is of the key
    five = plan.consts.index(5)                                   # the weight 5 is no constant of the layout itself
    rec = next(r for r in plan.records.tolist() if r[0] == WP.CONST and five in plan.pool[r[5]:r[5] + r[1]].tolist())
    at = plan.pool[rec[5]:rec[5] + rec[1]].tolist().index(five)
    cell = int(plan.pool[rec[4] + at])
    col, row = cell >> circuit.k, cell & ((1 << circuit.k) - 1)
    assert adv[col][row] == 5
    bad = [list(a) for a in adv]
    bad[col][row] = 6
    assert any("adv%d,%d)" % (col, row) in f for f in _named(MP.check(cs, bad, fixed, inst, copies)))
    # one fixed cell per distinct value, counted by the dummy pass; another weight is another key
    values = {v % EL.R for v in circuit.flat_params()}
    assert circuit.settings.total_const_size == len(values | {0, 1, 128}) and values <= {v for c in fixed[:len(circuit.gc.const_cols)] for v in c}
    weights = [list(r) for r in VC.WEIGHTS]
    weights[2][1] += 1
    other = VC.mlp(("Private", "Fixed", "Public"), weights=weights).keygen_inputs(VC.X)
    assert other[1] == fixed and other[2] != copies               # 2 -> 3, a value the circuit has already: the same fixed cells, other copy cycles
    weights[2][1] = 77
    other = VC.mlp(("Private", "Fixed", "Public"), weights=weights).keygen_inputs(VC.X)
    assert other[1] != fixed                                      # a value it has not: another fixed column
    weights[2][1] = 3
    private = VC.mlp(VC.DEFAULT), VC.mlp(VC.DEFAULT, weights=weights)
    assert private[0].keygen_inputs(VC.X)[1] == private[1].keygen_inputs(VC.X)[1]     # private parameters are in no key


@pytest.mark.parametrize("k, w, dims, options", [(6, 2, [3, 4], {}), (7, 2, [11, 11], {}), (9, 2, [16, 16, 16], {}), (9, 1, [5, 7, 3], dict(relu_last=False)),
                                                 (9, 2, [5, 7, 3], dict(relu_first=True)), (10, 3, [7, 8, 5], dict(rebase=[4, 128])),
                                                 (10, 2, [9, 6], dict(rebase=[3], relu_last=False)), (8, 2, [3], dict(relu_first=True))])
def test_the_constant_count_of_fixed_parameters_is_the_dummy_passes(k, w, dims, options):
    """total_const_size is counted from the parameters and a miniature of the circuit (MlpCircuit._own_constants): it must be what a
    dummy pass over the circuit itself counts, with and without rebase, ReLU first / last, widths that pad a dot and widths that do not"""
    import numpy as np
    from ezkl_amd import ezkl_layout as EL
    rng = np.random.default_rng(3)
    weights = [rng.integers(-3, 4, (dims[i + 1], dims[i])).tolist() for i in range(len(dims) - 1)]
    biases = [rng.integers(-5, 6, dims[i + 1]).tolist() for i in range(len(dims) - 1)]
    for vis in (("Private", "Fixed", "Public"), ("Public", "Fixed", "KZGCommit")):
        circuit = EL.MlpCircuit(k, w, weights, biases, VC.BASE, VC.LEGS, n_inputs=dims[0], visibility=vis, **options)
        roomy = EL.MlpCircuit(k, w, weights, biases, VC.BASE, VC.LEGS, n_inputs=dims[0], visibility=vis, total_const_size=16 + circuit.n_params, **options)
        reg = EL.BaseRegion(roomy.gc, False)
        roomy.layout(reg, [EL.Val(0)] * dims[0], EL.Val)
        assert circuit.settings.total_const_size == len(reg.const_order)
        assert circuit.fresh().settings.total_const_size == circuit.settings.total_const_size


@pytest.mark.parametrize("tri", VC.TRIPLES, ids=VC.ids)
def test_the_plan_replays_to_the_layouts_columns(tri):
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    for weights, biases, inputs in ((VC.WEIGHTS, VC.BIASES, [VC.X, [0, 0, 0], [-9, -1, -30]]), (VC.UNIT_WEIGHTS, VC.UNIT_BIASES, VC.EDGE_INPUTS)):
        circuit = VC.mlp(tri, weights, biases)
        plan = WP.record_plan(circuit)
        WP.validate(plan)
        assert WP.WitnessPlan.from_bytes(plan.to_bytes()) == plan
        head = WP.peek(plan.to_bytes())
        assert head["n_advice"] == len(circuit.gc.cs.advice) == N_MODEL_COLUMNS + _shape(tri)[0] and head["param_hash"] == WP.params_hash(circuit)
        assert {int(r[0]) for r in plan.records} <= {WP.COPY, WP.CONST, WP.INPUT, WP.PARAM, WP.ADD, WP.SUB, WP.MUL, WP.HINT, WP.RCIDX, WP.INVZ, WP.DOT}
        for x in inputs:
            adv, inst = circuit.witness(x)
            cols, outs = WP.run_plan_host(plan, x)
            assert len(cols) == len(adv)
            for c, (mine, ref) in enumerate(zip(cols, adv)):
                assert mine == ref, "advice column %d differs" % c
            assert [v % EL.R for v in outs] == circuit.outputs and circuit.instances(x, outs) == inst
    for x in VC.OVER_INPUTS:                                      # one past the bound: refused by the layout and by the replay, in the same words
        with pytest.raises(AssertionError, match="value exceeds the decomposition range"):
            circuit.witness(x)
        with pytest.raises(AssertionError, match="value exceeds the decomposition range"):
            WP.run_plan_host(plan, x)


def _files(tmp_path, tri):
    from ezkl_amd import execute as X
    path = tmp_path / ("%s.json" % VC.ids(tri))
    path.write_text(json.dumps(VC.description(tri)))
    described, _ = X._load_circuit(str(path))
    parsed = VC.compiled(tri, described.settings.total_const_size, described.settings.total_assignments)
    return str(path), described, X._build_mlp(X._describe_compiled(parsed))


@pytest.mark.parametrize("tri", VC.TRIPLES, ids=VC.ids)
def test_a_description_and_a_compiled_graph_load_into_the_same_circuit(tmp_path, tri):
    from ezkl_amd import execute as X, plonk as P, witness_plan as WP
    path, described, compiled = _files(tmp_path, tri)
    direct = VC.mlp(tri)
    assert described.visibility == compiled.visibility == tri
    a, b, c = (circ.keygen_inputs(VC.X) for circ in (described, compiled, direct))
    assert P.serialize_cs(a[0]) == P.serialize_cs(b[0]) == P.serialize_cs(c[0]) and a[1] == b[1] == c[1] and a[2] == b[2] == c[2]
    assert WP.params_hash(described) == WP.params_hash(compiled) == WP.params_hash(direct)
    assert WP.record_plan(described).to_bytes() == WP.record_plan(compiled).to_bytes()
    # gen_witness on the host: the outputs are the circuit's whatever is visible; without an SRS a committed tensor has an empty module result
    w = X.gen_witness(path, {"input_data": [[float(v) for v in VC.X]]})
    assert [int.from_bytes(bytes.fromhex(h), "little") for h in w["outputs"][0]] == [29, 0, 19, 17]
    for key, v in zip(("processed_inputs", "processed_params", "processed_outputs"), tri):
        assert w[key] == ({"poseidon_hash": None, "polycommit": None} if v == "KZGCommit" else None)


def test_a_compiled_graph_whose_module_sizes_disagree_is_refused():
    from ezkl_amd import execute as X
    tri = ("KZGCommit", "Private", "Public")
    parsed = VC.compiled(tri, 4, 262)
    parsed["settings"]["module_sizes"]["polycommit"] = [4]
    with pytest.raises(ValueError, match="module sizes"):
        X._build_mlp(X._describe_compiled(parsed))


HASHED = {"Hashed": {"hash_is_public": True, "outlets": []}}


@pytest.mark.parametrize("key, value, words", [("input_visibility", HASHED, "input is Hashed"), ("param_visibility", HASHED, "params is Hashed"),
                                               ("output_visibility", HASHED, "output is Hashed"), ("input_visibility", "Fixed", "input is Fixed"),
                                               ("output_visibility", "Private", "output is Private"), ("output_visibility", "Fixed", "output is Fixed"),
                                               ("param_visibility", "Public", "params is Public")])
def test_what_is_outside_the_triples_is_refused_by_name(tmp_path, key, value, words):
    from ezkl_amd import execute as X, ezkl_layout as EL
    desc = VC.description(VC.DEFAULT)
    desc["run_args"][key] = value
    path = tmp_path / "m.json"
    path.write_text(json.dumps(desc))
    for call in (lambda: X._load_circuit(str(path)), lambda: X.gen_witness(str(path), {"input_data": [[1.0, 2.0, 3.0]]})):
        with pytest.raises(ValueError, match="unsupported visibility: " + words):
            call()
    ra = desc["run_args"]
    parsed = VC.compiled((ra["input_visibility"], ra["param_visibility"], ra["output_visibility"]), 4, 262)
    for any_visibility in (False, True):                         # the compiled form: from the loader, and from gen_witness's reader
        with pytest.raises(ValueError, match="unsupported visibility: " + words):
            d = X._describe_compiled(parsed, any_visibility)
            EL.visibility_triple(d["visibility"])


def test_a_plan_of_another_triple_is_recorded_again(tmp_path):
    """a .wplan next to the key that was written for another triple of the same model is not replayed"""
    from ezkl_amd import execute as X, witness_plan as WP
    a, b = VC.mlp(("Public", "Private", "Public")), VC.mlp(VC.DEFAULT)
    assert len(a.gc.cs.advice) == len(b.gc.cs.advice) and a.n_inputs == b.n_inputs          # only the hash tells them apart
    pk = str(tmp_path / "pk.key")
    blob_a, blob_b = WP.record_plan(a).to_bytes(), WP.record_plan(b).to_bytes()
    assert blob_a != blob_b
    open(pk + ".wplan", "wb").write(blob_a)
    assert X._plan_for(a, pk) == blob_a and X._plan_for(b, pk) == blob_b
    c = VC.mlp(("KZGCommit", "Private", "Public"))
    assert X._plan_for(c, pk) == WP.record_plan(c).to_bytes() and WP.peek(X._plan_for(c, pk))["n_advice"] == len(a.gc.cs.advice) + 1


TWO = VC.TRIPLES


@pytest.mark.parametrize("tri", TWO, ids=VC.ids)
def test_parameters_that_span_two_columns(tri):
    """132 parameters at k = 7 (122 rows a column): the module of the parameters is two unblinded columns, the second begins with
    parameter 122; mock and plan replay as on the base case"""
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    weights, biases, x, k, w = VC.two_column()
    circuit = VC.mlp(tri, weights, biases, k, w)
    cs, fixed, copies, adv, inst, fails = _checked(circuit, x)
    assert fails == []
    model_columns = len(VC.mlp(VC.DEFAULT, weights, biases, k, w).gc.cs.advice)
    modules = {what: var for what, var, _ in circuit.committed()}
    n_module_columns = sum(var.num_blocks() for var in modules.values())
    assert cs.unblinded == list(range(n_module_columns)) and cs.n_advice == model_columns + n_module_columns
    if tri[1] == "KZGCommit":
        var, flat = modules["params"], [v % EL.R for v in circuit.flat_params()]
        assert len(flat) == 132 and var.num_blocks() == 2 and var.col_size == 122
        first, second = (adv[blk[0].index] for blk in var.inner)
        assert first[:122] == flat[:122] and not any(first[122:]) and second[:10] == flat[122:] and not any(second[10:])
        bad = [list(a) for a in adv]
        bad[var.inner[1][0].index][9] = (second[9] + 1) % EL.R
        assert _named(MP.check(cs, bad, fixed, inst, copies))
    plan = WP.record_plan(circuit)
    WP.validate(plan)
    for xs in (x, [0] * 11, [-v for v in x]):
        cols, outs = WP.run_plan_host(plan, xs)
        want, inst = circuit.witness(xs)
        assert cols == want and circuit.instances(xs, outs) == inst


def _proof_file(path, proof, instances=((1, 2),)):
    from ezkl_amd import codecs
    open(path, "w").write(codecs.write_proof_json(proof, [list(c) for c in instances]))


def _witness_file(path, groups):
    """groups: per processed_* key a list of (x, y), or None"""
    from ezkl_amd import codecs
    hexed = lambda pts: None if pts is None else {"poseidon_hash": None, "polycommit": [[{"x": codecs.felt_to_hex_le(x), "y": codecs.felt_to_hex_le(y)} for x, y in pts]]}
    keys = ("processed_inputs", "processed_params", "processed_outputs")
    open(path, "w").write(json.dumps(dict({"inputs": [], "outputs": []}, **{k: hexed(g) for k, g in zip(keys, groups)})))


@pytest.mark.parametrize("count", [0, 1, 3])
def test_swap_proof_commitments_on_bytes(tmp_path, count):
    """exactly the first 64 x count bytes change, to the points as the EVM transcript writes them (32 bytes big-endian x, then y), in
    the order input, params, output; the rest, the other fields and the hex mirror agree"""
    from ezkl_amd import codecs, execute as X
    proof = bytes((7 * i + 3) % 256 for i in range(64 * 5 + 17))
    points = [(0x1234 + (i << 200), 0xabcdef + (i << 131)) for i in range(3)]
    groups = {0: (None, None, None), 1: (None, [points[1]], None), 3: ([points[0]], [points[1]], [points[2]])}[count]
    written = [p for g in groups if g for p in g]
    pf, wf = str(tmp_path / "proof.json"), str(tmp_path / "witness.json")
    _proof_file(pf, proof)
    _witness_file(wf, groups)
    before = json.loads(open(pf).read())
    res = X.swap_proof_commitments(pf, wf)
    after = json.loads(open(pf).read())
    new = bytes(after["proof"])
    head = b"".join(x.to_bytes(32, "big") + y.to_bytes(32, "big") for x, y in written)
    assert len(head) == 64 * count and new == head + proof[64 * count:] and len(new) == len(proof)
    assert after["hex_proof"] == "0x" + new.hex() and res["proof"] == new and res["commitments"] == count
    assert res["changed"] == (count > 0) and ("no commitments" in res["note"]) == (count == 0)
    assert {k: v for k, v in after.items() if k not in ("proof", "hex_proof")} == {k: v for k, v in before.items() if k not in ("proof", "hex_proof")}
    assert codecs.read_proof_json(open(pf).read())["instances"] == [[1, 2]]
    assert X.witness_commitments(wf) == written
    assert not X.swap_proof_commitments(pf, wf)["changed"]                    # a second swap of the same points changes nothing
    if count == 3:                                                            # the order is input, params, output whatever the file's key order
        w = json.loads(open(wf).read())
        open(wf, "w").write(json.dumps({k: w[k] for k in reversed(list(w))}))
        assert X.witness_commitments(wf) == written
        _proof_file(pf, proof[:100])
        with pytest.raises(ValueError, match="commitments"):
            X.swap_proof_commitments(pf, wf)
