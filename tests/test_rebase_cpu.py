"""The rebase division of the MLP family without a GPU: ezkl wraps every Gemm whose output scale grew in a RebaseScale whose integer
denominator is laid out by layouts.rs:219-267 `div` -- a claimed rounded quotient, range-checked, with |input - claim * d| < d enforced.
The rounding helper against f64::round, the layout against the oracle's MockProver, the recorded plan against the layout engine (the new
record kind DIVC through the host interpreter), the failures both validators and the interpreter must report, and `gen_witness` on a
description at ezkl's default scales."""
import json

import numpy as np
import pytest

from oracle import mock_prover as MP

BASE, LEGS = 128, 2
TOP = BASE ** LEGS - 1                                          # the largest value a decomposition holds
IDENTITY = [[int(i == j) for j in range(3)] for i in range(3)]
# identity weights, bias 0: the inputs are the dividends.  Per divisor: exact halves of either sign, their neighbours, zero, and the largest
# in-range value of either sign
DIVIDENDS = {4: [[2, -2, 6], [-6, 1, 0], [TOP, -TOP, 5]],
             3: [[1, 2, -2], [4, 5, 0], [TOP, -TOP, -4]],
             128: [[64, -64, 192], [-192, 63, 65], [TOP, -TOP, 0]]}


def _identity(d, w):
    from ezkl_amd import ezkl_layout as EL
    return EL.MlpCircuit(8 if w == 2 else 9, w, [IDENTITY], [[0, 0, 0]], BASE, LEGS, relu_last=False, rebase=[d])


def _two_layer():
    """3 -> 4 -> 2 with ReLU after both layers, weights and biases in +-127, both layers divided by 2^7"""
    from ezkl_amd import ezkl_layout as EL
    rng = np.random.default_rng(7)
    Ws = [rng.integers(-127, 128, (4, 3)).tolist(), rng.integers(-127, 128, (2, 4)).tolist()]
    bs = [rng.integers(-127, 128, 4).tolist(), rng.integers(-127, 128, 2).tolist()]
    return EL.MlpCircuit(9, 2, Ws, bs, BASE, LEGS, rebase=[128, 128]), Ws, bs


CASES = {"identity_d%d_w%d" % (d, w): (lambda d=d, w=w: (_identity(d, w), DIVIDENDS[d])) for d in (4, 3, 128) for w in (1, 2)}
CASES["two_layer_relu_last_d128"] = lambda: (_two_layer()[0], [[100, -128, 77], [-5, 0, 127]])


def _rounded(s, d):
    """the rule in words: |s| / d rounded half up, with the sign of s"""
    q, r = divmod(abs(s), d)
    q += 2 * r >= d
    return q if s >= 0 else -q


def _forward(Ws, bs, rebase, x, relu_last=True):
    """an integer forward pass of its own: Gemm, rounded division, bias, ReLU"""
    v = np.array(x, dtype=object)
    for i, (W, b, d) in enumerate(zip(Ws, bs, rebase)):
        v = np.array([_rounded(int(t), d) for t in np.array(W, dtype=object) @ v], dtype=object) + np.array(b, dtype=object)
        if i + 1 < len(Ws) or relu_last:
            v = np.array([max(int(t), 0) for t in v], dtype=object)
    return [int(t) for t in v]


def test_rounding_is_f64_round_as_exact_integers():
    from ezkl_amd import execute as X, ezkl_layout as EL
    for s, d, q in ((2, 4, 1), (-2, 4, -1), (6, 4, 2), (-6, 4, -2), (1, 4, 0), (0, 4, 0), (1, 3, 0), (2, 3, 1), (-2, 3, -1), (4, 3, 1), (5, 3, 2)):
        assert EL.round_div(s, d) == q == X._rust_round(s / d), (s, d)
    rng = np.random.default_rng(11)
    for d in (2, 3, 128, 16384, 1000003, 2 ** 32 - 1):
        samples = [int(v) for v in rng.integers(-(1 << 52) + 1, 1 << 52, 300)] + [(1 << 52) - 1, -(1 << 52) + 1]
        for m in [0, 1, 2] + [int(v) for v in rng.integers(0, ((1 << 52) - 1) // d - 1, 60)]:        # at and around a half boundary
            for e in (-1, 0, 1):
                s = m * d + d // 2 + e
                samples += [s, -s]
        for s in samples:
            assert abs(s) < 1 << 52
            assert EL.round_div(s, d) == X._rust_round(s / d) == _rounded(s, d), (s, d)
    with pytest.raises(AssertionError, match="rebase dividend outside the exact-division range"):
        EL.round_div(1 << 52, 2)
    assert EL.ConvMnistConfig(10, 16, (-64, 64), 4).div(-6) == -2                     # the conv circuit's Div table is the same helper


def _quotient_cells(circuit):
    """(column, row) of every claimed quotient: the destinations of the plan's DIVC records"""
    from ezkl_amd import witness_plan as WP
    plan = WP.record_plan(circuit)
    cells = [int(c) for r in plan.records.tolist() if r[0] == WP.DIVC for c in plan.pool[r[4]:r[4] + r[1]]]
    return [(c >> circuit.k, c & ((1 << circuit.k) - 1)) for c in cells]


@pytest.mark.parametrize("name", list(CASES))
def test_mock_prover_accepts_the_layout_and_refuses_another_quotient(name):
    from ezkl_amd import ezkl_layout as EL
    circuit, xs = CASES[name]()
    cs, fixed, copies, reg = circuit.keygen_inputs(xs[0])
    assert reg.linear <= circuit.settings.total_assignments
    for x in xs:
        adv, inst = circuit.witness(x)
        assert MP.check(cs, adv, fixed, inst, copies) == [], x
        if name.startswith("identity"):
            d = circuit.rebase[0]
            assert [EL.signed(v) for v in inst[0]] == [_rounded(s, d) for s in x]
    cells = _quotient_cells(circuit)
    assert len(cells) == sum(len(W) for W in circuit.weights)
    adv, inst = circuit.witness(xs[0])
    for col, row in (cells[0], cells[-1]):
        for delta in (1, -1):
            bad = [list(a) for a in adv]
            bad[col][row] = (bad[col][row] + delta) % EL.R
            assert MP.check(cs, bad, fixed, inst, copies), "a claimed quotient off by %d went through" % delta


def test_a_consistent_witness_of_a_wrong_quotient_is_refused(monkeypatch):
    """every cell computed from a claim two off: only |input - claim * d| < d stands in its way"""
    from ezkl_amd import ezkl_layout as EL
    circuit, xs = CASES["identity_d4_w2"]()
    cs, fixed, copies, _ = circuit.keygen_inputs(xs[0])
    right = EL.round_div
    monkeypatch.setattr(EL, "round_div", lambda s, d: right(s, d) + 2)
    adv, inst = circuit.witness(xs[0])
    assert [EL.signed(v) for v in inst[0]] == [_rounded(s, 4) + 2 for s in xs[0]]
    assert MP.check(cs, adv, fixed, inst, copies)


def test_the_two_layer_circuit_computes_the_integer_model():
    from ezkl_amd import ezkl_layout as EL
    circuit, Ws, bs = _two_layer()
    for x in CASES["two_layer_relu_last_d128"]()[1]:
        assert [EL.signed(v) for v in circuit.witness(x)[1][0]] == _forward(Ws, bs, [128, 128], x)
    assert circuit.fresh().rebase == [128, 128]
    with pytest.raises(ValueError, match="rebase"):
        EL.MlpCircuit(9, 2, Ws, bs, BASE, LEGS, rebase=[128])
    with pytest.raises(ValueError, match="rebase"):
        EL.MlpCircuit(9, 2, Ws, bs, BASE, LEGS, rebase=[128, 0])


@pytest.mark.parametrize("name", list(CASES))
def test_host_interpreter_reproduces_the_layout_engine(name):
    from ezkl_amd import witness_plan as WP
    circuit, xs = CASES[name]()
    plan = WP.record_plan(circuit)
    assert WP.DIVC in plan.records[:, 0].tolist() and WP.KIND_NAMES[WP.DIVC] == "div" and WP.DIVC == 15
    assert WP.WitnessPlan.from_bytes(plan.to_bytes()) == plan
    for x in xs:
        adv, inst = circuit.witness(x)
        cols, outs = WP.run_plan_host(plan, x)
        for c, (mine, ref) in enumerate(zip(cols, adv)):
            assert mine == ref, "advice column %d differs" % c
        assert len(cols) == len(adv) and [outs] == inst


def test_records_follow_the_ops_not_the_width_and_the_hash_follows_the_rebase():
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    def mlp(width, rebase):
        W = [[int(i == j) for j in range(width)] for i in range(width)]
        return EL.MlpCircuit(9, 2, [W], [[0] * width], BASE, LEGS, rebase=rebase)
    narrow, wide = WP.record_plan(mlp(3, [4])), WP.record_plan(mlp(7, [4]))
    assert narrow.n_records == wide.n_records and narrow.n_cells < wide.n_cells
    plain, ones = mlp(3, None), mlp(3, [1])
    assert WP.record_plan(plain).to_bytes() == WP.record_plan(ones).to_bytes()
    assert WP.params_hash(plain) == WP.params_hash(ones) and plain.plan_identity() == ones.plan_identity()
    assert WP.DIVC not in WP.record_plan(ones).records[:, 0].tolist()
    assert WP.params_hash(mlp(3, [128])) not in (WP.params_hash(plain), WP.params_hash(mlp(3, [4])))
    assert WP.record_plan(mlp(3, [128])).param_hash == WP.params_hash(mlp(3, [128]))


def div_plan(count, d, k=9):
    """a hand-built plan: an INPUT record into column 0, one DIVC record from there into column 1; the outputs are the quotients"""
    from ezkl_amd import witness_plan as WP
    n = 1 << k
    idx = np.arange(count, dtype=np.uint32)
    pool = np.concatenate([idx, idx, n + idx, idx])
    records = [[WP.INPUT, count, 0, 0, 0, count, 0, 0], [WP.DIVC, count, d, 0, 2 * count, 3 * count, 0, 0]]
    return WP.WitnessPlan(k, 2, count, [], [], records, n + idx, pool, 2 * count, 2, b"\0" * 32)


def test_a_dividend_beyond_the_exact_range_is_refused_by_name():
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    plan = div_plan(5, 3)
    x = [7, -(1 << 52) + 1, (1 << 52) - 1, 0, -8]
    cols, outs = WP.run_plan_host(plan, x)
    assert [EL.signed(v) for v in outs] == [_rounded(s, 3) for s in x] == [EL.signed(v) for v in cols[1][:5]]
    for bad in (1 << 52, -(1 << 52)):
        with pytest.raises(AssertionError, match=r"rebase dividend outside the exact-division range \(div record 1, element 3"):
            WP.run_plan_host(plan, [7, 1, 2, bad, bad])


def test_a_zero_divisor_is_refused_by_both_validators_and_the_upload():
    import ctypes as C
    from ezkl_amd import lib, native, witness_plan as WP
    L, H = native.load(), lib.load()
    good, bad = div_plan(4, 1), div_plan(4, 0)
    WP.validate(good)
    blob = good.to_bytes()
    assert L.ezkl_prover_witness_plan_check(blob, C.c_size_t(len(blob))) == 0
    with pytest.raises(WP.PlanError, match="zero divisor"):
        WP.validate(bad)
    with pytest.raises(WP.PlanError, match="zero divisor"):
        WP.run_plan_host(bad, [1, 2, 3, 4])
    blob = bad.to_bytes()
    assert L.ezkl_prover_witness_plan_check(blob, C.c_size_t(len(blob))) == -3
    assert "zero divisor" in L.ezkl_prover_last_error().decode() and "(div)" in L.ezkl_prover_last_error().decode()
    h = C.c_void_p()
    assert H.ezkl_hip_witness_plan_upload(blob, C.c_size_t(len(blob)), C.byref(h)) == -3 and not h.value      # refused before a device is asked for
    assert "zero divisor" in H.ezkl_hip_witness_last_error().decode()
    later = div_plan(4, 2)                                        # a kind past the last one is still unknown, and a div source is a read
    later.records = later.records.copy()
    later.records[1, 0] = WP.DIVC + 1
    with pytest.raises(WP.PlanError, match="unknown kind"):
        WP.validate(later)
    blob = later.to_bytes()
    assert L.ezkl_prover_witness_plan_check(blob, C.c_size_t(len(blob))) == -3 and "unknown kind" in L.ezkl_prover_last_error().decode()
    unread = div_plan(4, 2)
    unread.pool = unread.pool.copy()
    unread.pool[3 * 4] = 100                                      # a source cell no record has written
    with pytest.raises(WP.PlanError, match="read before"):
        WP.validate(unread)
    blob = unread.to_bytes()
    assert L.ezkl_prover_witness_plan_check(blob, C.c_size_t(len(blob))) == -3 and "read before" in L.ezkl_prover_last_error().decode()


def description(tmp_path, name="rebase.compiled.json", logrows=9, **over):
    """a description at ezkl's default scales: input_scale = param_scale = 7, every Gemm divided by 2^7 -> (path, weights, biases)"""
    _, Ws, bs = _two_layer()
    ra = dict(logrows=logrows, num_inner_cols=2, decomp_base=BASE, decomp_legs=LEGS, input_scale=7, param_scale=7)
    j = {"model": "mlp", "run_args": ra, "weights": Ws, "biases": bs, "rebase": [128, 128]}
    j.update(over)
    path = tmp_path / name
    path.write_text(json.dumps(j))
    return str(path), Ws, bs


def test_gen_witness_at_the_default_scales(tmp_path):
    from ezkl_amd import codecs, execute as X, ezkl_layout as EL
    compiled, Ws, bs = description(tmp_path)
    x = [0.7734375, -1.0, 0.6015625]                              # 99, -128, 77 at scale 7
    w = X.gen_witness(compiled, {"input_data": [x]}, output=str(tmp_path / "witness.json"))
    parsed = codecs.read_witness_json(open(tmp_path / "witness.json").read())
    want = _forward(Ws, bs, [128, 128], [99, -128, 77])
    assert [EL.signed(v) for v in parsed["inputs"][0]] == [99, -128, 77]
    assert [EL.signed(v) for v in parsed["outputs"][0]] == want and any(want)
    assert w["pretty_elements"]["rescaled_outputs"] == [[codecs.rust_f64_to_string(v / 128.0) for v in want]]
    assert w["pretty_elements"]["rescaled_inputs"] == [[codecs.rust_f64_to_string(v) for v in x]]
    circuit, _ = X._load_circuit(compiled)
    assert circuit.rebase == [128, 128] and [EL.signed(v) for v in circuit.witness([99, -128, 77])[1][0]] == want
    # a divisor that is no power of two: the output scale must be said
    odd, _, _ = description(tmp_path, "odd.json", rebase=[128, 100])
    with pytest.raises(ValueError, match="output_scale"):
        X.gen_witness(odd, {"input_data": [x]})
    said, _, _ = description(tmp_path, "said.json", rebase=[128, 100], output_scale=7)
    w = X.gen_witness(said, {"input_data": [x]})
    want = _forward(Ws, bs, [128, 100], [99, -128, 77])
    assert w["pretty_elements"]["rescaled_outputs"] == [[codecs.rust_f64_to_string(v / 128.0) for v in want]]
    with pytest.raises(ValueError, match="rebase"):
        X.gen_witness(description(tmp_path, "short.json", rebase=[128])[0], {"input_data": [x]})
    # a quotient the decomposition cannot hold: weights of 2^21 leave 99 * 2^21 / 2 above 128^2
    big = [[[1 << 21, 0, 0]] * 4, Ws[1]]
    wide, _, _ = description(tmp_path, "wide.json", weights=big, rebase=[2, 128], output_scale=7)
    with pytest.raises(ValueError, match="decomposition range"):
        X.gen_witness(wide, {"input_data": [x]})
    # without "rebase" a description is what it was: scale 0 throughout
    plain, _, _ = description(tmp_path, "plain.json")
    j = json.load(open(plain)); del j["rebase"]
    open(plain, "w").write(json.dumps(j))
    assert X._read_compiled(plain)[0]["in_scale"] == 0 and X._load_circuit(plain)[0].rebase == [1, 1]
