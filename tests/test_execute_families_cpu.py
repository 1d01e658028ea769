"""`execute` on conv, norm and pooled-classifier descriptions, without a device: a description round-trips to the circuit it was written
from; the seeded parameters of ConvMnistCircuit / PoolClassifierCircuit are what they were; every malformed field, every other
visibility and an unknown model are refused by name; `gen_witness` on the host gives the circuit's outputs and the lookup statistics a
test computes on its own; `witness_plan.lookup_stats_host` over the replayed plan agrees with the layout; the MLP's bytes are unchanged."""
import json
import os

import numpy as np
import pytest

import execute_family_cases as F
import witness_synth as S

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _signed_outputs(w):
    from ezkl_amd import ezkl_layout as EL
    return [EL.signed(int.from_bytes(bytes.fromhex(o), "little")) for o in w["outputs"][0]]


def _settings(c):
    s = c.gc.settings
    return (s.logrows, s.num_inner_cols, s.total_assignments, s.total_const_size, s.required_range_checks, [n for n, _ in s.required_lookups], s.lookup_range,
            s.model_instance_shapes, s.total_dynamic_col_size, s.num_dynamic_lookups, s.total_shuffle_col_size, s.num_shuffles, len(c.gc.cs.advice))


@pytest.mark.parametrize("name", list(F.CASES))
def test_a_description_round_trips_to_the_circuit_it_describes(tmp_path, name):
    from ezkl_amd import execute as X, witness_plan as WP
    make, xs, _ = F.CASES[name]
    direct = make()
    path = F.write_description(X, direct, tmp_path / "c.json", input_scale=0, output_scale=0)
    loaded, parsed = X._load_circuit(path)
    assert type(loaded) is type(direct) and parsed["model"] == {"conv": "conv", "norm": "norm", "pool": "pool_classifier"}[name.split("_")[0]]
    assert loaded.plan_identity() == direct.plan_identity() and WP.params_hash(loaded) == WP.params_hash(direct)
    assert _settings(loaded) == _settings(direct) and loaded.n_inputs == direct.n_inputs
    fresh = loaded.fresh()
    assert fresh is not loaded and fresh.gc.cs is not loaded.gc.cs and fresh.plan_identity() == direct.plan_identity() and _settings(fresh) == _settings(direct)
    if hasattr(direct, "model"):
        assert loaded.model(xs[0]) == direct.model(xs[0])
    assert X.describe(loaded) == X.describe(direct)


def test_the_seeded_parameters_are_what_they_were():
    from ezkl_amd import ezkl_layout as EL
    c = EL.ConvMnistCircuit()
    rng = np.random.default_rng(0)
    kernels, fc_w, fc_b = rng.integers(-20, 21, (4, 5, 5)), rng.integers(-12, 13, (10, 576)), rng.integers(-40, 41, 10)
    assert (c.kernels == kernels).all() and not c.conv_bias.any() and (c.fc_w == fc_w).all() and (c.fc_b == fc_b).all()
    given = EL.ConvMnistCircuit(kernels=kernels, conv_bias=[0] * 4, fc_w=fc_w.tolist(), fc_b=fc_b)
    assert given.plan_identity() == c.plan_identity() == c.fresh().plan_identity()
    one = EL.ConvMnistCircuit(fc_b=list(range(10)))                             # the other three keep their seeded values
    assert (one.kernels == kernels).all() and (one.fc_w == fc_w).all() and one.fc_b.tolist() == list(range(10))
    c.kernels = c.kernels + 1                                                    # (tests set parameters this way too: `fresh` carries them)
    assert c.fresh().plan_identity() == c.plan_identity() != given.plan_identity()
    for pool in ("max", "sum"):
        p = EL.PoolClassifierCircuit(10, 2, 12000, pool=pool)
        rng = np.random.default_rng(0)
        want = [rng.integers(-4, 5, (2, 3, 3)), rng.integers(-8, 9, 2), rng.integers(-4, 5, (4, 18)), rng.integers(-16, 17, 4)]
        assert all((a == b).all() for a, b in zip((p.kernels, p.conv_bias, p.fc_w, p.fc_b), want))
        again = EL.PoolClassifierCircuit(10, 2, 12000, pool=pool, kernels=want[0], conv_bias=want[1], fc_w=want[2], fc_b=want[3])
        assert again.plan_identity() == p.plan_identity() == p.fresh().plan_identity()


def _broken(j, path, value):
    """a copy of the description with the field at `path` replaced (None: removed)"""
    j = json.loads(json.dumps(j))
    at = j
    for key in path[:-1]:
        at = at[key]
    if value is None:
        del at[path[-1]]
    else:
        at[path[-1]] = value
    return j


MALFORMED = {
    "conv_k6": [(("image",), 0), (("image",), "6"), (("kernel",), 7), (("kernel",), None), (("out_channels",), 1.5), (("stride",), -1), (("classes",), None),
                (("denom",), 0), (("lookup_range",), [5, 1]), (("lookup_range",), [0]), (("capacity",), 0), (("kernels",), [[[3, 3, 3]] * 2]), (("kernels",), None),
                (("conv_bias",), [0, 0]), (("fc_w",), [[1, 2, 3, 4]]), (("fc_w",), [[1, 2, 3, 4.5], [1, 2, 3, 4]]), (("fc_b",), [1]), (("fc_b",), [1, 1 << 70]),
                (("run_args", "logrows"), None), (("run_args", "num_inner_cols"), 0), (("run_args", "decomp_base"), 1), (("run_args", "decomp_legs"), "2"),
                (("run_args", "input_scale"), 0.5), (("run_args",), [1])],
    "norm_softmax": [(("rows",), 0), (("length",), None), (("input_scale",), 0), (("output_scale",), 1.5), (("eps",), 0), (("eps",), "small"), (("layer_norm",), 1),
                     (("lookup_range",), [0, -255]), (("capacity",), None)],
    "pool_max": [(("pool",), "mean"), (("pool_size",), 0), (("pool_size",), 7), (("pool_stride",), None), (("capacity",), -5), (("fc_w",), [[0] * 17] * 4),
                 (("conv_bias",), 3), (("kernel",), 9)],
}


@pytest.mark.parametrize("name", list(MALFORMED))
def test_every_malformed_field_is_refused_by_name(tmp_path, name):
    from ezkl_amd import execute as X
    good = X.describe(F.CASES[name][0]())
    path = tmp_path / "c.json"
    for where, value in MALFORMED[name]:
        path.write_text(json.dumps(_broken(good, where, value)))
        with pytest.raises(ValueError, match=where[-1]) as e:
            X._load_circuit(str(path))
        assert type(e.value) is ValueError, (where, value)
        with pytest.raises(ValueError, match=where[-1]):                         # the same refusal at the witness end
            X.gen_witness(str(path), F.data(F.CASES[name][1][0]))


def test_an_unknown_model_and_any_other_visibility_are_refused_by_name(tmp_path):
    from ezkl_amd import execute as X
    path = tmp_path / "c.json"
    for model in ("einsum", "surrogate", "sort_topk", None, 7):
        path.write_text(json.dumps({"model": model, "run_args": {}}))
        for call in (lambda: X._load_circuit(str(path)), lambda: X.gen_witness(str(path), {"input_data": [[0.0]]})):
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == "unsupported compiled circuit: %r" % (model,)
    for name in ("conv_k6", "norm_softmax", "pool_sum"):
        make, xs, _ = F.CASES[name]
        good = X.describe(make())
        for key, what, value, named in (("input_visibility", "input", "Public", "Public"), ("input_visibility", "input", "KZGCommit", "KZGCommit"),
                                        ("param_visibility", "params", "KZGCommit", "KZGCommit"), ("param_visibility", "params", "Fixed", "Fixed"),
                                        ("output_visibility", "output", "Private", "Private"), ("output_visibility", "output", "KZGCommit", "KZGCommit"),
                                        ("output_visibility", "output", {"Hashed": {"hash_is_public": True, "outlets": []}}, "Hashed")):
            path.write_text(json.dumps(_broken(good, ("run_args", key), value)))
            for call in (lambda: X._load_circuit(str(path)), lambda: X.gen_witness(str(path), F.data(xs[0]))):
                with pytest.raises(ValueError, match="unsupported visibility: %s is %s" % (what, named)):
                    call()


@pytest.mark.parametrize("name", list(F.CASES))
def test_gen_witness_on_the_host_outputs_and_statistics(tmp_path, name):
    from ezkl_amd import execute as X, ezkl_layout as EL, witness_plan as WP
    make, xs, refused = F.CASES[name]
    circuit = make()
    path = F.write_description(X, circuit, tmp_path / "c.json", input_scale=0, output_scale=3)
    plan = WP.record_plan(make())
    for i, x in enumerate(xs):
        out = tmp_path / ("w%d.json" % i)
        w = X.gen_witness(path, F.data(x), output=str(out))
        assert json.loads(out.read_text()) == w and X.gen_witness(path, F.data(x), synthesis="host") == w
        assert w["inputs"] == [[(v % EL.R).to_bytes(32, "little").hex() for v in x]]
        if hasattr(circuit, "model"):
            assert _signed_outputs(w) == circuit.model(x)
        adv, inst = make().witness(x)
        assert [[int.from_bytes(bytes.fromhex(o), "little") for o in w["outputs"][0]]] == inst
        want = F.expected_stats(name, circuit, x)
        assert (w["min_lookup_inputs"], w["max_lookup_inputs"]) == want, "the layout's statistics against the test's own"
        cols, outs = WP.run_plan_host(plan, x)
        assert cols == adv and WP.lookup_stats_host(plan, cols) == want
        assert w["max_range_size"] == circuit.base - 1 == max(hi - lo for lo, hi in circuit.gc.settings.required_range_checks)
        assert w["pretty_elements"]["rescaled_outputs"] == [[X.codecs.rust_f64_to_string(v / 8.0) for v in _signed_outputs(w)]]
        if not any(x):
            assert want == (0, 0) or name in ("conv_k10",)                      # all zeros: no lookup input but 0 (conv_k10: its conv bias)
    if name == "conv_k10":
        assert F.expected_stats(name, circuit, xs[2]) == (0, 5)                  # the positive conv bias alone: every lookup input >= 0, the minimum stays 0
    if name == "norm_softmax":
        lo, hi = F.expected_stats(name, circuit, xs[1])                          # every lookup input <= 0, the row maxima at 0: the maximum stays 0
        assert lo < 0 and hi == 0
    if refused is not None:
        with pytest.raises(ValueError, match="lookup input -?[0-9]+ outside the table range") as e:
            X.gen_witness(path, F.data(refused))
        assert type(e.value) is ValueError
        with pytest.raises(AssertionError, match="lookup input outside the table range"):
            WP.run_plan_host(plan, refused)
    with pytest.raises(ValueError, match="input shape"):
        X.gen_witness(path, F.data(xs[0][:-1]))
    with pytest.raises(ValueError, match="synthesis"):
        X.gen_witness(path, F.data(xs[0]), synthesis="gpu")


def test_lookup_stats_host_on_planted_sources():
    """what no circuit of these families produces: every lookup input negative (the maximum stays 0), every one positive, the table
    bounds themselves, a source beyond 62 bits, no lookup record at all"""
    from ezkl_amd import witness_plan as WP
    def plan_of(vals, lo=-5000, hi=5000):
        b = S.Builder(8, 2)
        src = b.input(b.fresh(len(vals), corner=True), vals)
        b.lookup(b.fresh(len(vals)), src, b.table(lo, 2501, list(range(lo, hi + 1))))
        return b.plan(), b.x
    for vals, want in (([-3, -1, -4999, -7], (-4999, 0)), ([3, 1, 4999, 7], (0, 4999)), ([-5000, 5000], (-5000, 5000)), ([0, 0, 0], (0, 0)), ([-2], (-2, 0))):
        plan, x = plan_of(vals)
        assert WP.lookup_stats_host(plan, WP.run_plan_host(plan, x)[0]) == want == (min(0, *vals), max(0, *vals))
    plan, x = plan_of([1, 2, 3])
    cols, _ = WP.run_plan_host(plan, x)
    cell = int(plan.pool[plan.records[1, 5] + 1])
    cols[cell >> 8][cell & 255] = (-(1 << 62)) % S.R
    with pytest.raises(ValueError, match=WP.STATS_ERROR):
        WP.lookup_stats_host(plan, cols)
    cols[cell >> 8][cell & 255] = (-(1 << 62) + 1) % S.R
    assert WP.lookup_stats_host(plan, cols) == (-(1 << 62) + 1, 3)
    case = S.elementwise_case(65, "permuted", 1)
    assert WP.lookup_stats_host(case.plan, case.columns()) == (0, 0)


def test_the_mlp_bytes_are_unchanged_and_its_family_is_in_the_table(tmp_path):
    from ezkl_amd import execute as X
    out = tmp_path / "witness.json"
    X.gen_witness(os.path.join(G, "model_k6.compiled"), os.path.join(G, "input_k6.json"), output=str(out))
    assert out.read_bytes() == open(os.path.join(G, "witness_k6.json"), "rb").read()
    out2 = tmp_path / "witness2.json"
    X.gen_witness(os.path.join(G, "model_k6.compiled"), os.path.join(G, "input_k6.json"), output=str(out2), synthesis="host", pk_path=None)
    assert out2.read_bytes() == out.read_bytes()
    assert set(X.FAMILIES) == {"mlp", "conv", "pool_classifier", "norm"}
    circuit, _ = X._load_circuit(os.path.join(G, "model_k6.compiled"))
    assert type(circuit).__name__ == "MlpCircuit" and X._max_range_size(circuit) == 127
