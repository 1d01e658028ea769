#!/usr/bin/env python3
"""What a batch costs at the file level: `m` inferences of one MLP as ONE proof of a batched circuit (execute "mlp_batch": every Gemm a
Freivalds einsum, second-phase advice) next to the same `m` inferences as `m` batch-1 proofs in an MlpCircuit session, in one sitting.

    python tools/batch_mlp_bench.py --batch 10 --layers 9 --width 100 --tag TAG [--dir DIR] [--timeout SECONDS]

The defaults are examples/onnx/large_mlp as the reference states it: 9 x Linear(100, 100) + ReLU on a 10 x 100 batch.  The weights are
seeded integers of that shape (entries in [-16, 16], biases and inputs in [-128, 128]: values at scale 7), every layer is rebased by
2^7, and each circuit sits at the smallest logrows that holds it: the range table fits, the einsum columns stay one block and there are
at most 64 advice columns.  Children, each a process of its own under its own `timeout -k 10`; one that fails ends the run:
  make      both descriptions, one SRS per logrows, `setup` of both (timed), `gen_witness` of the batch on the host and from phase 0
            of the plan next to the key (timed, the bytes compared), the m batch-1 witness files (row i of the batch's outputs compared)
  batch     one `execute.Prover` on the batched circuit: its `opened` stages, the first proof, then the median of the rest by stage
            and by phase (device milliseconds of the plan's replay)
  rows      one `execute.Prover` on the batch-1 circuit: the m proofs of the m rows, by stage, and their sum
Every proof is verified.  Result: profiles/<tag>_batch_mlp.json.  There is no threshold: the numbers are reported, not judged."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
BASE, LEGS, SCALE, SEED0 = 1024, 2, 7, 7


def _files(d):
    f = lambda name: os.path.join(d, name)
    return dict(batch=f("batch.json"), rows=f("rows.json"), vk_batch=f("vk_batch.key"), pk_batch=f("pk_batch.key"), vk_rows=f("vk_rows.key"), pk_rows=f("pk_rows.key"),
                meta=f("meta.json"))


def _med(xs):
    return round(statistics.median(xs), 6) if xs else None


def _network(a):
    import numpy as np
    rng = np.random.default_rng(1)
    weights = [rng.integers(-16, 17, (a.width, a.width)).tolist() for _ in range(a.layers)]
    biases = [rng.integers(-128, 129, a.width).tolist() for _ in range(a.layers)]
    x = rng.integers(-128, 129, a.batch * a.width).tolist()
    return weights, biases, x


def _smallest_logrows(make, at_least):
    """the smallest logrows >= at_least at which make(logrows) configures with at most 64 advice columns"""
    for k in range(at_least, 25):
        try:
            circuit = make(k)
        except (AssertionError, ValueError):
            continue                                                            # an einsum column would need a second block
        if len(circuit.gc.cs.advice) <= 64:
            return circuit
    raise SystemExit("no logrows up to 24 holds the circuit")


def make(a, d):
    from ezkl_amd import execute as X, ezkl_layout as EL
    weights, biases, x = _network(a)
    rebase = [1 << SCALE] * a.layers
    fs, t = _files(d), {}
    least = BASE.bit_length()                                                   # the range table's rows and the blinding rows fit
    batch = _smallest_logrows(lambda k: EL.BatchMlpCircuit(k, 1, a.batch, weights, biases, BASE, LEGS, rebase=rebase), least)
    rows = _smallest_logrows(lambda k: EL.MlpCircuit(k, 1, weights, biases, BASE, LEGS, rebase=rebase), least)
    scales = dict(input_scale=SCALE, param_scale=SCALE)
    j = X.describe(batch, input_scale=SCALE, output_scale=SCALE)
    j["run_args"].update(scales)
    json.dump(j, open(fs["batch"], "w"))
    json.dump(dict(model="mlp", run_args=dict(logrows=rows.k, num_inner_cols=1, decomp_base=BASE, decomp_legs=LEGS, **scales), weights=weights, biases=biases,
                   rebase=rebase, total_assignments=rows.settings.total_assignments), open(fs["rows"], "w"))
    info = {}
    for name, circuit in (("batch", batch), ("rows", rows)):
        srs = os.path.join(d, "kzg%d.srs" % circuit.k)
        if not os.path.exists(srs):
            t0 = time.perf_counter(); X.gen_srs(srs, circuit.k, secret=0x5eed + circuit.k); t["gen_srs_k%d" % circuit.k] = time.perf_counter() - t0
        t0 = time.perf_counter(); info[name] = X.setup(fs[name], srs, fs["vk_" + name], fs["pk_" + name]); t["setup_" + name] = time.perf_counter() - t0
        info[name].update(logrows=circuit.k, wplan_bytes=os.path.getsize(fs["pk_" + name] + ".wplan"))
    real = [v / (1 << SCALE) for v in x]                                        # the data file holds reals: quantized at input_scale
    host_s, device_s = [], []
    for i in range(3):
        out = os.path.join(d, "witness_batch.json")
        t0 = time.perf_counter(); w = X.gen_witness(fs["batch"], {"input_data": [real]}, output=out); host_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); X.gen_witness(fs["batch"], {"input_data": [real]}, output=out + ".dev", synthesis="device", pk_path=fs["pk_batch"]); device_s.append(time.perf_counter() - t0)
        if open(out, "rb").read() != open(out + ".dev", "rb").read():
            raise SystemExit("gen_witness: the device's file differs from the host's")
    rows_s = []
    for i in range(a.batch):
        t0 = time.perf_counter()
        wi = X.gen_witness(fs["rows"], {"input_data": [real[i * a.width:(i + 1) * a.width]]}, output=os.path.join(d, "witness_row%d.json" % i))
        rows_s.append(time.perf_counter() - t0)
        if wi["outputs"][0] != w["outputs"][0][i * a.width:(i + 1) * a.width]:
            raise SystemExit("row %d of the batch's outputs differs from the batch-1 circuit's" % i)
    json.dump(dict(batch=a.batch, layers=a.layers, width=a.width, k_batch=batch.k, k_rows=rows.k), open(fs["meta"], "w"))
    print(json.dumps(dict(seconds={n: round(v, 3) for n, v in t.items()}, setup=info, gen_witness_batch_host_s=[round(v, 4) for v in host_s],
                          gen_witness_batch_device_s=[round(v, 4) for v in device_s], gen_witness_rows_host_s_sum=round(sum(rows_s), 4),
                          gen_witness_bytes_equal=True, rows_equal_the_batch=True)))


def _session(d, which, witnesses, proofs):
    from ezkl_amd import execute as X
    fs = _files(d)
    meta = json.load(open(fs["meta"]))
    srs = os.path.join(d, "kzg%d.srs" % meta["k_" + which])
    walls, reports = [], []
    t0 = time.perf_counter()
    with X.Prover(fs[which], fs["pk_" + which], srs) as p:
        open_s = time.perf_counter() - t0
        for i in range(proofs):
            how, out = {}, os.path.join(d, "proof_%s%d.json" % (which, i))
            t0 = time.perf_counter()
            p.prove(witnesses[i % len(witnesses)], out, seed=SEED0 + i, report=how)
            walls.append(time.perf_counter() - t0)
            reports.append(how)
            if not X.verify(out, fs[which], fs["vk_" + which], srs):
                raise SystemExit("%s proof %d does not verify" % (which, i))
        opened = dict(p.opened)
    return open_s, opened, walls, reports


def _by_stage(reports):
    return {s: _med([r["stages"].get(s, 0.0) for r in reports]) for s in sorted({s for r in reports for s in r["stages"]})}


def batch(a, d):
    open_s, opened, walls, reports = _session(d, "batch", [os.path.join(d, "witness_batch.json")], a.proofs)
    rest = reports[1:]
    phases = sorted({ph for r in rest for ph in r.get("phase_ms", {})})
    print(json.dumps(dict(synthesis_paths=sorted({r["path"] for r in reports}), open_s=round(open_s, 4), opened={n: round(v, 4) for n, v in opened.items()},
                          prove_first_s=round(walls[0], 4), prove_rest_median_s=_med(walls[1:]), stages_rest_median_s=_by_stage(rest),
                          phase_device_ms_rest_median={str(ph): _med([r["phase_ms"][ph] for r in rest if ph in r.get("phase_ms", {})]) for ph in phases},
                          create_proof_breakdown_rest_median_s={s: _med([r["create_proof_breakdown"].get(s, 0.0) for r in rest])
                                                                for s in sorted({s for r in rest for s in r["create_proof_breakdown"]})})))


def rows(a, d):
    witnesses = [os.path.join(d, "witness_row%d.json" % i) for i in range(a.batch)]
    open_s, opened, walls, reports = _session(d, "rows", witnesses, a.batch + 1)       # the first proof warms the session; then the m rows
    print(json.dumps(dict(synthesis_paths=sorted({r["path"] for r in reports}), open_s=round(open_s, 4), opened={n: round(v, 4) for n, v in opened.items()},
                          prove_first_s=round(walls[0], 4), prove_row_median_s=_med(walls[1:]), prove_rows_sum_s=round(sum(walls[1:]), 4),
                          stages_row_median_s=_by_stage(reports[1:]), replay_device_ms_row_median=_med([r.get("device_ms", 0.0) for r in reports[1:]]))))


def _child(args, seconds, env):
    """one child, one process, one time limit; -> its last JSON line"""
    cmd = ["timeout", "-k", "10", str(int(seconds)), sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise SystemExit("%s ended with status %d: nothing more is started" % (" ".join(cmd), r.returncode))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--layers", type=int, default=9)
    ap.add_argument("--width", type=int, default=100)
    ap.add_argument("--proofs", type=int, default=5, help="proofs of the batched circuit in its session (the first is reported apart)")
    ap.add_argument("--tag")
    ap.add_argument("--dir", help="where the artefacts go (default: a temporary directory, removed afterwards)")
    ap.add_argument("--timeout", type=int, default=600, help="seconds for each child process")
    ap.add_argument("--child", choices=["make", "batch", "rows"])
    a = ap.parse_args()
    if a.child:
        {"make": make, "batch": batch, "rows": rows}[a.child](a, a.dir)
        return
    if not a.tag:
        ap.error("--tag is needed")
    env = dict(os.environ, ENABLE_HIP_GPU="1")                                   # the gate open: "auto" makes the witness on the device
    d = a.dir or tempfile.mkdtemp(prefix="batch_mlp_")
    os.makedirs(d, exist_ok=True)
    common = ["--batch", str(a.batch), "--layers", str(a.layers), "--width", str(a.width), "--proofs", str(a.proofs), "--dir", d]
    out = dict(tag=a.tag, batch=a.batch, layers=a.layers, width=a.width, proofs=a.proofs, decomp_base=BASE, decomp_legs=LEGS, scale=SCALE)
    try:
        for name in ("make", "batch", "rows"):
            out[name] = _child(["--child", name] + common, a.timeout, env)
            print(name, json.dumps(out[name]), flush=True)
        path = os.path.join(ROOT, "profiles", a.tag + "_batch_mlp.json")
        json.dump(out, open(path, "w"), indent=1)
        print("written to %s" % path)
    finally:
        if not a.dir:
            shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
