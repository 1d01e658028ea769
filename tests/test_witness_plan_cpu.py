"""Witness plans without a GPU (ezkl_amd/witness_plan.py): the layout of an MlpCircuit recorded once and replayed by the host
interpreter `run_plan_host` -- the executable specification of the device kernels -- must reproduce `circuit.witness(x)` exactly, in every
advice column and in the outputs, on circuits whose columns overflow into further blocks (the duplicated rows of `dot`), with one and two
inner columns, with and without layers.  The blob is deterministic, round-trips, and the validator -- the Python mirror and the C++ check
the upload runs (csrc/witness_plan.hpp, through libezkl_prover.so: no device needed) -- refuses what a kernel must never index with."""
import os

import numpy as np
import pytest

import fixture_k6 as FX


def _mlp(k, w, layers=3, width=16, seed=3, **kw):
    from ezkl_amd import ezkl_layout as EL
    rng = np.random.default_rng(seed)
    Ws = [rng.integers(-3, 4, (width, width)).tolist() for _ in range(layers)]
    bs = [rng.integers(-5, 6, width).tolist() for _ in range(layers)]
    return EL.MlpCircuit(k, w, Ws, bs, 128, 2, **kw), rng.integers(-9, 10, width).tolist()


def _mlp_k7(w):
    """dots of 16 / w steps in columns of 122 usable rows: running sums cross column tops (the duplicated row inside `dot`)"""
    from ezkl_amd import ezkl_layout as EL
    rng = np.random.default_rng(5)
    Ws = [rng.integers(-3, 4, (8, 16)).tolist(), rng.integers(-3, 4, (4, 8)).tolist()]
    bs = [rng.integers(-5, 6, 8).tolist(), rng.integers(-5, 6, 4).tolist()]
    return EL.MlpCircuit(7, w, Ws, bs, 128, 2), rng.integers(-9, 10, 16).tolist()


def _golden():
    from ezkl_amd import codecs, execute as X, ezkl_layout as EL
    circuit, _ = X._load_circuit(os.path.join(FX.G, "model_k6.compiled"))
    w = codecs.read_witness_json(open(os.path.join(FX.G, "witness_k6.json")).read())
    return circuit, [v if v < EL.R // 2 else v - EL.R for v in w["inputs"][0]]


def _relu_only(w, relu_last=True):
    from ezkl_amd import ezkl_layout as EL
    return EL.MlpCircuit(8, w, [], [], 128, 2, n_inputs=3, relu_first=True, relu_last=relu_last), [5, -7, 0]


CASES = {
    "golden_k6_5_blocks": _golden,
    "mlp_k9_w2_3_blocks": lambda: _mlp(9, 2),
    "mlp_k9_w1_5_blocks": lambda: _mlp(9, 1),
    "1l_relu_k8": lambda: _relu_only(2),
    "mlp_k9_w2_no_relu_last_2_blocks": lambda: _mlp(9, 2, relu_last=False),
    "1l_relu_k8_w1": lambda: _relu_only(1),
    "mlp_k7_w1_dot_crosses_a_column_top": lambda: _mlp_k7(1),
    "mlp_k7_w2_dot_crosses_a_column_top": lambda: _mlp_k7(2),
}


@pytest.mark.parametrize("name", list(CASES))
def test_host_interpreter_reproduces_the_layout_engine(name):
    from ezkl_amd import witness_plan as WP
    circuit, x = CASES[name]()
    adv, inst = circuit.witness(x)
    plan = WP.record_plan(circuit)
    cols, outs = WP.run_plan_host(plan, x)
    assert len(cols) == len(adv) == plan.n_advice
    for c, (mine, ref) in enumerate(zip(cols, adv)):
        assert mine == ref, "advice column %d differs" % c
    assert [outs] == inst
    # the plan writes every cell the layout writes: no non-zero cell outside it, and the launch count is that of the layout-op calls
    assert plan.n_cells >= sum(1 for col in adv for v in col if v)
    assert plan.n_records <= plan.n_ops + 8, "one record per batch of like ops, not one per row or per dot step"
    if name == "golden_k6_5_blocks":
        assert circuit.gc.advices[0].num_blocks() == 5
    if name.startswith("mlp_k7"):                                 # a dot step without products: the duplicated running sum
        dups = 0
        for kind, count, w, steps, dst, a, b, _ in plan.records.tolist():
            if kind == WP.DOT:
                d = plan.pool[dst:dst + count * steps].reshape(steps, count)
                aa = plan.pool[a:a + count * steps * w].reshape(steps, w, count)
                dups += int(((d != WP.NONE) & (aa == WP.NONE).all(1)).sum())
        assert dups >= 1


def test_block_counts_of_the_cases():
    """the cases are the ones that cross block boundaries"""
    for (circuit, x), blocks, cells in ((_mlp(9, 2), 3, 2082), (_mlp(9, 1), 5, 2081), (_mlp(9, 2, relu_last=False), 2, 1824), (_relu_only(2), 1, 141)):
        assert circuit.gc.advices[0].num_blocks() == blocks and circuit.synthesize(x).linear == cells


def test_another_input_same_plan():
    from ezkl_amd import witness_plan as WP
    circuit, x = _mlp(9, 2)
    plan = WP.record_plan(circuit)
    for x2 in ([0] * 16, [-9] * 16, list(range(-8, 8))):
        adv, inst = circuit.witness(x2)
        cols, outs = WP.run_plan_host(plan, x2)
        assert cols == adv and [outs] == inst


def test_recording_is_deterministic_and_round_trips():
    from ezkl_amd import witness_plan as WP
    circuit, x = _mlp(9, 2)
    blob = WP.record_plan(circuit).to_bytes()
    assert WP.record_plan(circuit).to_bytes() == blob
    again = WP.record_plan(_mlp(9, 2)[0]).to_bytes()             # a second circuit object with the same parameters
    assert again == blob
    plan = WP.WitnessPlan.from_bytes(blob)
    assert plan.to_bytes() == blob and plan == WP.record_plan(circuit)
    assert plan.param_hash == WP.params_hash(circuit) != WP.params_hash(_mlp(9, 2, seed=4)[0])
    assert WP.run_plan_host(plan, x)[0] == circuit.witness(x)[0]
    head = np.frombuffer(blob[:48], "<u4")
    assert head[0] == WP.MAGIC and head[1] == WP.VERSION and head[2] == 9 and head[3] == plan.n_advice
    with pytest.raises(WP.PlanError, match="version"):
        WP.WitnessPlan.from_bytes(blob[:4] + (2).to_bytes(4, "little") + blob[8:])
    with pytest.raises(WP.PlanError, match="bytes"):
        WP.WitnessPlan.from_bytes(blob[:-4])


def test_value_outside_the_decomposition_range_raises():
    from ezkl_amd import witness_plan as WP
    circuit, _ = _relu_only(2)
    plan = WP.record_plan(circuit)
    with pytest.raises(AssertionError, match="value exceeds the decomposition range"):
        circuit.witness([128 * 128, 0, 0])
    with pytest.raises(AssertionError, match="value exceeds the decomposition range.*decompose"):
        WP.run_plan_host(plan, [128 * 128, 0, 0])
    with pytest.raises(AssertionError, match="value exceeds the decomposition range"):
        WP.run_plan_host(plan, [0, -128 * 128, 0])
    cols, outs = WP.run_plan_host(plan, [128 * 128 - 1, -(128 * 128 - 1), 0])
    assert outs == [128 * 128 - 1, 0, 0]


def test_out_of_scope_circuits_are_refused_by_name():
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    with pytest.raises(WP.PlanError, match="SumProdCircuit"):
        WP.record_plan(EL.SumProdCircuit(8, 1, 400))
    reg = WP.RecordingRegion(_relu_only(2)[0].gc)
    for op, args in (("nonlinearity", ([], "exp")), ("sum", ([],)), ("prod", ([],)), ("dynamic_lookup", ([], [])), ("shuffle", ([], []))):
        with pytest.raises(WP.PlanError, match=op):
            getattr(reg, op)(*args)


def _beyond_the_recorder():
    """MlpCircuits the host engine lays out and the recorder refuses: (circuit, input, the refusal)"""
    from ezkl_amd import ezkl_layout as EL
    wide = EL.MlpCircuit(10, 2, [], [], 16384, 5, n_inputs=3, relu_first=True)                 # ezkl's default base with 5 legs: 2^70
    big = EL.MlpCircuit(8, 2, [[[1 << 70, 0, 0]] * 4], [[0, 0, 0, 0]], 128, 2)                  # a weight beyond int64 (times a zero input)
    return [(wide, [5, -7, 0], "decomposition range beyond 62 bits"), (big, [0, 0, 0], "a parameter beyond int64")]


def test_circuits_beyond_the_recorder_keep_the_host_path(monkeypatch, tmp_path):
    """the recorder refuses them by name; `execute` treats that as "no plan": "auto" takes the host path, only "device" raises"""
    from ezkl_amd import execute as X, witness_plan as WP
    monkeypatch.setenv("ENABLE_HIP_GPU", "1")
    monkeypatch.setenv("HIP_SMALL_K", "4")                        # the gate is open for every circuit here
    for circuit, x, why in _beyond_the_recorder():
        adv, inst = circuit.witness(x)                            # the host engine handles it
        assert len(adv) == len(circuit.gc.cs.advice)
        with pytest.raises(WP.PlanError, match=why):
            WP.record_plan(circuit)
        with pytest.raises(WP.PlanError, match=why):
            X._plan_for(circuit, str(tmp_path / "none.key"))
        assert X._device_witness(circuit, str(tmp_path / "none.key"), x, "auto") is None
        with pytest.raises(WP.PlanError, match=why):
            X._device_witness(circuit, str(tmp_path / "none.key"), x, "device")


def _tampered(plan):
    from ezkl_amd import witness_plan as WP
    q = WP.WitnessPlan.from_bytes(plan.to_bytes())
    q.pool, q.records = q.pool.copy(), q.records.copy()
    return q


def _bad_plans():
    """(what the validator must say, plan)"""
    from ezkl_amd import witness_plan as WP
    plan = WP.record_plan(_relu_only(2)[0])
    kinds = plan.records[:, 0].tolist()
    out = []
    q = _tampered(plan)                                           # a destination cell past the last column
    r = kinds.index(WP.COPY)
    q.pool[q.records[r, 4]] = plan.n_advice << plan.k
    out.append(("cell index out of range", q))
    q = _tampered(plan)                                           # a source cell past the last column
    q.pool[q.records[r, 5]] = 0xfffffff0
    out.append(("cell index out of range", q))
    q = _tampered(plan)                                           # a record that reads what only a LATER record writes
    later = int(plan.pool[plan.records[-1, 4]])
    q.pool[q.records[r, 5]] = later
    out.append(("read before", q))
    q = _tampered(plan)                                           # a record that reads its own destination
    r = kinds.index(WP.MUL)
    q.pool[q.records[r, 5]] = q.pool[q.records[r, 4]]
    out.append(("read before", q))
    q = _tampered(plan)                                           # a cell written twice
    q.pool[q.records[1, 4]] = q.pool[q.records[0, 4]]
    out.append(("written twice", q))
    q = _tampered(plan)                                           # an input index past the inputs
    q.pool[q.records[kinds.index(WP.INPUT), 5]] = plan.n_inputs
    out.append(("table index out of range", q))
    q = _tampered(plan)                                           # a constant index past the table
    q.pool[q.records[kinds.index(WP.CONST), 5]] = len(plan.consts)
    out.append(("table index out of range", q))
    q = _tampered(plan)                                           # an index array that runs past the pool
    q.records[2, 1] = len(plan.pool) + 1
    out.append(("past the pool", q))
    q = _tampered(plan)                                           # a dot step that reads an unwritten cell
    r = kinds.index(WP.DOT)
    q.pool[q.records[r, 5]] = later
    out.append(("read before", q))
    q = _tampered(plan)                                           # a dot product with its first operand missing
    q.pool[q.records[r, 5]] = WP.NONE
    out.append(("a product with one operand", q))
    q = _tampered(plan)
    q.records[3, 0] = 99
    out.append(("unknown kind", q))
    return plan, out


def test_validator_refuses_bad_blobs():
    from ezkl_amd import witness_plan as WP
    plan, bad = _bad_plans()
    WP.validate(plan)
    for what, q in bad:
        with pytest.raises(WP.PlanError, match=what):
            WP.validate(q)
        with pytest.raises(WP.PlanError, match=what):
            WP.run_plan_host(q, [1, 2, 3])


def test_c_validator_agrees_with_the_python_mirror():
    """csrc/witness_plan.hpp -- what ezkl_hip_witness_plan_upload runs before anything reaches the device -- through libezkl_prover.so (host
    code only; tools/asan_run.sh runs this under the sanitizers), and through the upload itself, which refuses a bad blob before it asks
    for a device"""
    import ctypes as C
    from ezkl_amd import lib, native, witness_plan as WP
    L, H = native.load(), lib.load()
    plan, bad = _bad_plans()
    check = lambda blob: L.ezkl_prover_witness_plan_check(blob, C.c_size_t(len(blob)))
    for circuit in (_mlp(9, 1)[0], _golden()[0]):
        assert check(WP.record_plan(circuit).to_bytes()) == 0
    assert check(plan.to_bytes()) == 0
    for what, q in bad:
        blob = q.to_bytes()
        assert check(blob) == -3, what
        assert what in L.ezkl_prover_last_error().decode(), (what, L.ezkl_prover_last_error())
        h = C.c_void_p()
        assert H.ezkl_hip_witness_plan_upload(blob, C.c_size_t(len(blob)), C.byref(h)) == -3 and not h.value
        assert what in H.ezkl_hip_witness_last_error().decode()
    blob = plan.to_bytes()
    for cut in (0, 10, 111, len(blob) - 1):
        assert check(blob[:cut]) == -3
    assert check(blob + b"\0") == -3
    assert check(blob[:4] + (7).to_bytes(4, "little") + blob[8:]) == -3 and "version" in L.ezkl_prover_last_error().decode()
    huge = bytearray(blob); huge[16:20] = (0xffffffff).to_bytes(4, "little")          # a record count that does not fit the blob
    assert check(bytes(huge)) == -3


def test_validators_on_a_sparse_plan():
    """a few hundred cells in columns of 2^18 rows: both validators keep their written-set by the pool (memory bounded by the blob, not by
    the geometry the header claims) and still catch what they catch on a dense plan; a header that claims 2^32 cells costs nothing"""
    import ctypes as C
    from ezkl_amd import ezkl_layout as EL, native, witness_plan as WP
    L = native.load()
    check = lambda blob: L.ezkl_prover_witness_plan_check(blob, C.c_size_t(len(blob)))
    circuit = EL.MlpCircuit(18, 2, [], [], 128, 2, n_inputs=3, relu_first=True)
    plan = WP.record_plan(circuit)
    assert WP._Written(plan.n_advice << plan.k, plan.pool).keys is not None          # the sparse form
    WP.validate(plan)
    assert check(plan.to_bytes()) == 0
    assert WP.run_plan_host(plan, [5, -7, 0])[1] == circuit.witness([5, -7, 0])[1][0]
    kinds = plan.records[:, 0].tolist()
    later = int(plan.pool[plan.records[-1, 4]])
    for what, edit in (("read before", lambda q: q.pool.__setitem__(q.records[kinds.index(WP.COPY), 5], later)),
                       ("written twice", lambda q: q.pool.__setitem__(q.records[1, 4], q.pool[q.records[0, 4]])),
                       ("read before", lambda q: q.pool.__setitem__(q.records[kinds.index(WP.COPY), 5], (1 << 18) - 1)),      # a cell no record writes
                       ("output cell is never written", lambda q: q.outputs.__setitem__(0, (1 << 18) - 2)),
                       ("cell index out of range", lambda q: q.pool.__setitem__(q.records[kinds.index(WP.COPY), 4], plan.n_advice << plan.k))):
        q = _tampered(plan)
        q.outputs = q.outputs.copy()
        edit(q)
        with pytest.raises(WP.PlanError, match=what):
            WP.validate(q)
        assert check(q.to_bytes()) == -3 and what in L.ezkl_prover_last_error().decode()
    q = _tampered(plan)                                           # k = 28 x 16 columns claimed by the header of the same small blob
    q.k, q.n_advice = 28, 16
    WP.validate(q)
    assert check(q.to_bytes()) == 0
    q = _tampered(plan)
    q.n_cells = len(plan.pool) + 1
    with pytest.raises(WP.PlanError, match="more cells than index words"):
        WP.validate(q)
    assert check(q.to_bytes()) == -3


def test_prove_refuses_an_unknown_synthesis_mode(tmp_path):
    """before it touches a file"""
    from ezkl_amd import execute as X
    with pytest.raises(ValueError, match="synthesis"):
        X.prove("none.json", "none.compiled", "none.key", str(tmp_path / "p.json"), "none.srs", synthesis="gpu")
