"""The contract's ONE JSON line must survive the driver's record (a 20 KB line came back `parsed: null`).
bench.compact_line() is a pure function of the full record, so it is sized here from records of real runs kept under profiles/."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (module level imports nothing that needs a GPU)

CONTRACT_KEYS = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"]


def _record(name):
    text = open(os.path.join(ROOT, "profiles", name)).read()
    lines = [l for l in text.splitlines() if l.startswith("{")]
    return json.loads(lines[-1] if lines else text)


@pytest.mark.parametrize("name, n", [("r05av_bench.log", 1), ("r05ax_bench_world8.json", 8)])
def test_line_is_short_and_round_trips(name, n):
    full = _record(name)
    if n == 8:
        full["n_gpus"] = 8                      # the kept record is 8 ranks sharing one device: n_gpus says 1 there
    text = bench.compact_line(full)
    assert "\n" not in text
    assert len(text) < bench.LINE_LIMIT < 8000
    line = json.loads(text)
    for k in CONTRACT_KEYS:
        assert k in line, k
    assert line["config"]["workload"].startswith("configs[1]")
    assert abs(line["value"] / full["value"] - 1) < 1e-4 and abs(line["ms_per_step"] / full["ms_per_step"] - 1) < 1e-4
    r = line["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic_source", "avg_launch_ms", "ntt", "product_peak", "kernels"):
        assert k in r, k
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-6
    assert r["ntt"]["elems_per_s"] > 0 and len(r["kernels"]) >= 2
    if n == 1:
        c = line["cpu_baseline"]
        for k in ("value", "unit", "cores", "kind", "sample", "ntt", "prove_seconds_k20_mlp"):
            assert k in c, k
        assert c["prove_seconds_k20_mlp"]["gpu"] == line["prove_seconds_k20_mlp"]["gpu"] > 0
        assert c["prove_seconds_k20_mlp"]["identical"] is True
    else:
        assert "rccl_ranks_seen" in line and line["prove_multi"]["all_ranks_same_proof"] is True
        assert "2^20" in line["msm_strong_scaling"]


def test_line_stays_short_whatever_the_legs_put_into_the_record():
    full = _record("r05av_bench.log")
    blob = "x" * 5000
    full["prove"]["einsum"]["error"] = blob
    full["prove"]["skipped"] = [blob] * 50
    full["roofline"]["traffic_source"] = blob
    full["cpu_baseline"]["sample"] = blob
    full["errors"] = [blob] * 10
    full["extra"]["msm_strong_scaling"] = {"error": blob}
    text = bench.compact_line(full)
    assert len(text) < bench.LINE_LIMIT
    line = json.loads(text)
    assert line["value"] > 0 and "roofline" in line and "cpu_baseline" in line


def test_emit_prints_one_line_and_keeps_the_full_record(tmp_path, capsys, monkeypatch):
    full = _record("r05av_bench.log")
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    bench.emit(full)
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and len(out) < bench.LINE_LIMIT
    assert json.load(open(tmp_path / "bench_full.json"))["prove"]["mlp_k20"]["prove_seconds_gpu"] == full["prove"]["mlp_k20"]["prove_seconds_gpu"]


def test_plain_run_line_has_no_placeholders_for_full_figures():
    """a plain run's record holds the headline and the figures of the two timed regions only: its line keeps the contract's keys and
    carries no empty entries for what --full measures"""
    full = _record("r05av_bench.log")
    plain = {k: full[k] for k in CONTRACT_KEYS + ["clock_warmup_steps", "extra"]}
    plain["roofline"] = {k: full["roofline"][k] for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "avg_launch_ms")}
    plain["roofline"]["ntt"] = {k: full["roofline"]["ntt"][k] for k in ("metric", "elems_per_s", "ms_per_step")}
    line = json.loads(bench.compact_line(plain))
    for k in CONTRACT_KEYS:
        assert k in line, k
    assert line["value"] == pytest.approx(full["value"], rel=1e-4) and line["ms_per_step"] == pytest.approx(full["ms_per_step"], rel=1e-4)
    assert set(line["roofline"]) == {"bound", "kernel", "achieved", "peak", "unit", "frac", "avg_launch_ms", "ntt"}
    assert set(line["roofline"]["ntt"]) == {"elems_per_s", "ms_per_step"}
    assert not {"cpu_baseline", "prove_seconds_k20_mlp", "prove_other_circuits", "prove_multi", "errors"} & set(line)


def test_multi_rank_line_carries_the_three_sharded_proofs():
    """N > 1: configs[3] (einsum, MLP k = 20) and configs[4] (the transformer surrogate at k = 22) each with what a SCALE run is checked by --
    seconds, same proof on every rank, verifier, rccl_ranks_seen -- and still a short line"""
    full = _record("r05ax_bench_world8.json")
    full["n_gpus"] = 8
    sub = {"prove_seconds_gpu": 0.31, "all_ranks_same_proof": True, "verifier_accepts": True, "rccl_ranks_seen": 8, "exchange_ms_per_proof_max": 4.2,
           "per_rank": [{"stats": {"x": "y" * 400}}] * 8}
    full["prove"]["rccl_ranks_seen"] = 8
    full["prove"]["mlp_k20"] = dict(sub)
    full["prove"]["transformer_k22"] = dict(sub, prove_seconds_gpu=0.25)
    text = bench.compact_line(full)
    assert len(text) < bench.LINE_LIMIT
    line = json.loads(text)
    assert line["rccl_ranks_seen"] == 8
    pm = line["prove_multi"]
    assert pm["mlp_k20"]["rccl_ranks_seen"] == 8 and pm["transformer_k22"]["prove_seconds_gpu"] == 0.25 and "per_rank" not in pm["transformer_k22"]
    # a leg that failed shows its error, shortened
    full["prove"]["transformer_k22"] = {"error": "z" * 3000}
    line = json.loads(bench.compact_line(full))
    assert len(line["prove_multi"]["transformer_k22"]["error"]) == 200 and len(bench.compact_line(full)) < bench.LINE_LIMIT


def test_dump_outputs_words_are_exact_and_bounded(tmp_path):
    """--dump-outputs: every 254-bit value leaves as its 32-bit words in float64, bit-exact; a dump over the size limit is refused"""
    import numpy as np
    rng = np.random.default_rng(1)
    limbs = rng.integers(0, 1 << 63, size=(5, 4), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    bench.dump_outputs(str(tmp_path / "out"), {"a": bench._words(limbs)})
    back = np.load(tmp_path / "out" / "a.npy")
    assert back.dtype == np.float64 and back.shape == (5, 8)
    assert (np.ascontiguousarray(back.astype(np.uint64).astype(np.uint32)).view(np.uint64).reshape(5, 4) == limbs).all()
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "big"), {"b": np.zeros(bench.DUMP_LIMIT_BYTES // 8 + 1)})
    assert not (tmp_path / "big").exists()
