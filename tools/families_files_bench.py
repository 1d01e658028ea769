#!/usr/bin/env python3
"""What the file level costs for a conv, norm or pooled-classifier circuit: `execute` on artefact files next to the class path that
`bench.py` uses (`circuit.witness` + `native.create_proof`), in one sitting.

    python tools/families_files_bench.py --family conv --k 17 --proofs 6 --tag TAG [--dir DIR] [--timeout SECONDS]

The circuit is written as this package's JSON description (execute.describe): conv = ConvMnistCircuit(logrows=k) with its seeded
parameters (k >= 17: its Div table has 65 537 rows), norm = a softmax NormCircuit of 2 x 4, pool = a max PoolClassifierCircuit of 8 x 8,
both with room for k.  Children, each a process of its own under its own `timeout -k 10`; one that fails ends the run:
  make     gen_srs, `setup` (timed), `gen_witness` on the host and from the plan next to the key (each timed per file; the bytes compared)
  stats    the plan replayed and its lookup statistics taken, several times: the replay's device_ms next to the statistics kernel's
           HIP-event time
  prove    `execute.prove` + `verify`, one call per proof
  session  one `execute.Prover`: its `opened` stages, the first proof, then the median of the rest by stage
  class    the same circuit through the class path: `circuit.witness` (the host layout), the columns to the device, `native.create_proof`
           on the key and bases the session loaded
Proofs are made at fixed seeds and their hashes compared across prove, session and class.  Result: profiles/<tag>_families.json.  There is
no threshold: the commit before these descriptions cannot read the files."""
import argparse
import hashlib
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
SEED0, N_WITNESSES = 7, 3


def _files(d):
    f = lambda name: os.path.join(d, name)
    return dict(compiled=f("circuit.json"), srs=f("kzg.srs"), vk=f("vk.key"), pk=f("pk.key"), meta=f("meta.json"))


def _circuit(family, k):
    from ezkl_amd import ezkl_layout as EL
    if family == "conv":
        return EL.ConvMnistCircuit(logrows=k), 16
    if family == "norm":
        return EL.NormCircuit(k, 2, 9 * 2 * (1 << k), 2, 4), 16
    return EL.PoolClassifierCircuit(k, 2, 9 * 2 * (1 << k), pool="max"), 16


def _med(xs):
    return round(statistics.median(xs), 6) if xs else None


def make(family, k, d):
    import numpy as np
    from ezkl_amd import execute as X
    circuit, hi = _circuit(family, k)
    rng = np.random.default_rng(3)
    fs, t = _files(d), {}
    json.dump(X.describe(circuit), open(fs["compiled"], "w"))
    t0 = time.perf_counter(); X.gen_srs(fs["srs"], k, secret=0x5eed); t["gen_srs"] = time.perf_counter() - t0
    t0 = time.perf_counter(); info = X.setup(fs["compiled"], fs["srs"], fs["vk"], fs["pk"]); t["setup"] = time.perf_counter() - t0
    host_s, device_s, equal = [], [], True
    for i in range(N_WITNESSES):
        data = {"input_data": [[float(v) for v in rng.integers(0, hi, circuit.n_inputs)]]}
        out = os.path.join(d, "witness%d.json" % i)
        t0 = time.perf_counter(); X.gen_witness(fs["compiled"], data, output=out); host_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); X.gen_witness(fs["compiled"], data, output=out + ".dev", synthesis="device", pk_path=fs["pk"]); device_s.append(time.perf_counter() - t0)
        equal = equal and open(out, "rb").read() == open(out + ".dev", "rb").read()
    sizes = {name: os.path.getsize(p) for name, p in fs.items() if os.path.exists(p)}
    sizes["wplan"] = os.path.getsize(fs["pk"] + ".wplan")
    json.dump(dict(family=family, k=k, setup=info, bytes=sizes), open(fs["meta"], "w"))
    print(json.dumps(dict(seconds={a: round(b, 3) for a, b in t.items()}, bytes=sizes, gen_witness_host_s=[round(v, 4) for v in host_s],
                          gen_witness_device_s=[round(v, 4) for v in device_s], gen_witness_bytes_equal=equal)))
    if not equal:
        raise SystemExit("gen_witness: the device's file differs from the host's")


def stats(d, rounds=7):
    from ezkl_amd import execute as X
    fs = _files(d)
    circuit, _ = X._load_circuit(fs["compiled"])
    w, x = X._read_witness(circuit, os.path.join(d, "witness0.json"), "device")
    dev = X._open_plan(circuit, fs["pk"], "device")
    cols = dev.alloc_columns()
    replay, kernel, got = [], [], None
    try:
        for _ in range(rounds):
            dev.run(x, columns=cols)
            replay.append(dev.last["device_ms"])
            got = dev.lookup_stats(cols)
            kernel.append(dev.last_stats_ms)
    finally:
        for c in cols:
            c.free()
        dev.free()
    ok = [got[0], got[1]] == [w["min_lookup_inputs"], w["max_lookup_inputs"]]
    print(json.dumps(dict(records=dev.n_records, lookup_records=dev.n_lookup_records, cells=dev.n_cells, launches=dev.last["launches"], min_max=list(got),
                          equals_the_witness_file=ok, replay_device_ms=dict(first=round(replay[0], 4), median_rest=_med(replay[1:])),
                          stats_kernel_ms=None if kernel[0] is None else dict(first=round(kernel[0], 4), median_rest=_med(kernel[1:])))))
    if not ok:
        raise SystemExit("the statistics differ from the witness file's")


def _hash(proof):
    return hashlib.sha256(proof).hexdigest()[:16]


def prove(d, proofs):
    from ezkl_amd import execute as X
    fs = _files(d)
    prove_s, verify_s, hashes, paths = [], [], [], set()
    for i in range(proofs):
        wit, out, how = os.path.join(d, "witness%d.json" % (i % N_WITNESSES)), os.path.join(d, "proof_a%d.json" % i), {}
        t0 = time.perf_counter(); proof = X.prove(wit, fs["compiled"], fs["pk"], out, fs["srs"], seed=SEED0 + i, report=how); prove_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); ok = X.verify(out, fs["compiled"], fs["vk"], fs["srs"]); verify_s.append(time.perf_counter() - t0)
        if not ok:
            raise SystemExit("proof %d does not verify" % i)
        hashes.append(_hash(proof))
        paths.add(how.get("path"))
    print(json.dumps(dict(synthesis_paths=sorted(paths), prove_first_s=round(prove_s[0], 4), prove_rest_median_s=_med(prove_s[1:]), verify_first_s=round(verify_s[0], 4),
                          verify_rest_median_s=_med(verify_s[1:]), proof_sha256=hashes)))


def session(d, proofs):
    from ezkl_amd import execute as X
    fs = _files(d)
    walls, reports, hashes = [], [], []
    t0 = time.perf_counter()
    with X.Prover(fs["compiled"], fs["pk"], fs["srs"]) as p:
        open_s = time.perf_counter() - t0
        for i in range(proofs):
            how = {}
            t0 = time.perf_counter()
            proof = p.prove(os.path.join(d, "witness%d.json" % (i % N_WITNESSES)), os.path.join(d, "proof_b%d.json" % i), seed=SEED0 + i, report=how)
            walls.append(time.perf_counter() - t0)
            reports.append(how)
            hashes.append(_hash(proof))
        opened = dict(p.opened)
    rest = reports[1:]
    stages = {s: _med([r["stages"].get(s, 0.0) for r in rest]) for s in sorted({s for r in rest for s in r["stages"]})}
    print(json.dumps(dict(synthesis_paths=sorted({r["path"] for r in reports}), open_s=round(open_s, 4), opened={a: round(b, 4) for a, b in opened.items()},
                          prove_first_s=round(walls[0], 4), prove_rest_median_s=_med(walls[1:]), stages_rest_median_s=stages,
                          replay_device_ms_rest_median=_med([r.get("device_ms", 0.0) for r in rest]), proof_sha256=hashes)))


def class_path(d, proofs):
    """bench.py's path: the circuit object, its host layout, create_proof -- on the key and the bases as a session loads them from the files"""
    from ezkl_amd import backend as B, execute as X, ezkl_layout as EL, native as NV
    fs = _files(d)
    circuit, _ = X._load_circuit(fs["compiled"])
    witness_s, columns_s, proof_s, hashes = [], [], [], []
    with X.Prover(fs["compiled"], fs["pk"], fs["srs"], synthesis="host") as p:
        for i in range(proofs):
            _, x = X._read_witness(circuit, os.path.join(d, "witness%d.json" % (i % N_WITNESSES)), "host")
            t0 = time.perf_counter(); adv, inst = circuit.witness(x); witness_s.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); cols = EL.cols_to_mont(adv, B); columns_s.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); proof = NV.create_proof(p.pk, p.bg, p.bgl, cols, seed=SEED0 + i, instances=inst, g2=p.g2, s_g2=p.s_g2); proof_s.append(time.perf_counter() - t0)
            hashes.append(_hash(proof))
    print(json.dumps(dict(circuit_witness_rest_median_s=_med(witness_s[1:]), columns_to_mont_rest_median_s=_med(columns_s[1:]), create_proof_first_s=round(proof_s[0], 4),
                          create_proof_rest_median_s=_med(proof_s[1:]), proof_sha256=hashes)))


def _child(args, seconds, env):
    """one child, one process, one time limit; -> its last JSON line"""
    cmd = ["timeout", "-k", "10", str(int(seconds)), sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise SystemExit("%s ended with status %d: nothing more is started" % (" ".join(cmd), r.returncode))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--family", choices=["conv", "norm", "pool"], default="conv")
    ap.add_argument("--k", type=int, default=17)
    ap.add_argument("--proofs", type=int, default=6)
    ap.add_argument("--tag")
    ap.add_argument("--dir", help="where the artefacts go (default: a temporary directory, removed afterwards)")
    ap.add_argument("--timeout", type=int, default=300, help="seconds for each child process")
    ap.add_argument("--child", choices=["make", "stats", "prove", "session", "class"])
    a = ap.parse_args()
    if a.child:
        {"make": lambda: make(a.family, a.k, a.dir), "stats": lambda: stats(a.dir), "prove": lambda: prove(a.dir, a.proofs), "session": lambda: session(a.dir, a.proofs),
         "class": lambda: class_path(a.dir, a.proofs)}[a.child]()
        return
    if not a.tag:
        ap.error("--tag is needed")
    env = dict(os.environ, ENABLE_HIP_GPU="1")                                   # the gate open: "auto" makes the witness on the device
    d = a.dir or tempfile.mkdtemp(prefix="families_files_")
    os.makedirs(d, exist_ok=True)
    common = ["--family", a.family, "--k", str(a.k), "--dir", d, "--proofs", str(a.proofs)]
    out = dict(tag=a.tag, family=a.family, k=a.k, proofs=a.proofs)
    try:
        for name in ("make", "stats", "prove", "session", "class"):
            out[name] = _child(["--child", name] + common, a.timeout, env)
            print(name, json.dumps(out[name]), flush=True)
        hs = [out[name]["proof_sha256"] for name in ("prove", "session", "class")]
        out["proof_bytes_equal_across_paths"] = all(h == hs[0] for h in hs)
        path = os.path.join(ROOT, "profiles", a.tag + "_families.json")
        json.dump(out, open(path, "w"), indent=1)
        print("written to %s" % path)
    finally:
        if not a.dir:
            shutil.rmtree(d, ignore_errors=True)
    if not out.get("proof_bytes_equal_across_paths"):
        raise SystemExit("proof bytes differ across the paths")


if __name__ == "__main__":
    main()
