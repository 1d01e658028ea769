#!/usr/bin/env python3
"""What a USER of the package waits for: `execute.prove` / `execute.verify` on artefact files, per call, against a resident
`execute.Prover` session on the same files.

    python tools/prove_files_bench.py --k 14 --k 17 --proofs 8 --tag TAG [--parent DIR] [--dir DIR] [--timeout SECONDS]

The circuit is the bench MLP (tools/bench_circuits.mlp_circuit) written as this package's JSON description; the artefacts are made with
execute.gen_srs / setup / gen_witness (not timed).
  leg A: execute.prove + execute.verify, one call per proof -- only calls every revision of the package has, so the same script measures
         an older checkout: --parent DIR (a built checkout of the parent commit) runs leg A of THIS file against that checkout's package
         (--root DIR in the child: nothing is written into the other tree), on the same files.  That run is the yardstick; leg A of this tree is never the baseline of this tree's leg B.
  leg B: (where execute.Prover exists) one session: its `opened` stages, the first proof, then median and minimum of the rest with
         the split by stage, and how much of the steady-state wall is the plan's replay (device_ms) plus create_proof.
Proofs are made at fixed seeds and their hashes compared across the legs.  Each size and each leg is a process of its own under its own
`timeout -k 10`; a leg that fails ends the run.  Result: profiles/<tag>_session.json.

    python tools/prove_files_bench.py --child structure --k 17
the structural pass alone, no GPU: the layout (execute._fresh_keygen_inputs) against execute._plonk_cs on the selector rows packed as
NativeProvingKey.set_selectors packs them, seconds of each, and whether gates and lookups are equal as pickles."""
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
SEED0 = 7
TREE = "this"                                        # which package a leg measured: this file's own tree, or --root's ("parent")


def _files(d):
    f = lambda name: os.path.join(d, name)
    return dict(compiled=f("model.compiled.json"), srs=f("kzg.srs"), vk=f("vk.key"), pk=f("pk.key"), meta=f("meta.json"))


def make(k, d, n_witnesses):
    """the artefacts of one size (not timed by the legs; their own wall is recorded)"""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_circuits as BC
    from ezkl_amd import execute as X
    rng = np.random.default_rng(1)
    circuit, x = BC.mlp_circuit(k, rng)
    fs, t = _files(d), {}
    json.dump({"model": "mlp", "run_args": dict(logrows=k, num_inner_cols=circuit.w, decomp_base=circuit.base, decomp_legs=circuit.legs),
               "weights": circuit.weights, "biases": circuit.biases, "total_assignments": circuit.settings.total_assignments}, open(fs["compiled"], "w"))
    t0 = time.time(); X.gen_srs(fs["srs"], k, secret=0x5eed); t["gen_srs"] = time.time() - t0
    t0 = time.time(); info = X.setup(fs["compiled"], fs["srs"], fs["vk"], fs["pk"]); t["setup"] = time.time() - t0
    t0 = time.time()
    for i in range(n_witnesses):
        xi = x if i == 0 else rng.integers(min(x), max(x) + 1, len(x)).tolist()
        X.gen_witness(fs["compiled"], {"input_data": [[float(v) for v in xi]]}, output=os.path.join(d, "witness%d.json" % i))
    t["gen_witness"] = time.time() - t0
    sizes = {name: os.path.getsize(p) for name, p in fs.items() if os.path.exists(p)}
    sizes["wplan"] = os.path.getsize(fs["pk"] + ".wplan") if os.path.exists(fs["pk"] + ".wplan") else 0
    json.dump(dict(k=k, n_witnesses=n_witnesses, layers=len(circuit.weights), width=len(circuit.weights[0]), setup=info, seconds=t, bytes=sizes), open(fs["meta"], "w"))
    print(json.dumps(dict(seconds={a: round(b, 3) for a, b in t.items()}, bytes=sizes)))


def _spread(xs):
    return dict(median=round(statistics.median(xs), 5), min=round(min(xs), 5), n=len(xs)) if xs else None


def leg_a(d, proofs):
    from ezkl_amd import execute as X
    fs, meta = _files(d), json.load(open(_files(d)["meta"]))
    prove_s, verify_s, hashes, paths = [], [], [], []
    for i in range(proofs):
        wit, out, how = os.path.join(d, "witness%d.json" % (i % meta["n_witnesses"])), os.path.join(d, "proof_a%d.json" % i), {}
        t0 = time.perf_counter()
        proof = X.prove(wit, fs["compiled"], fs["pk"], out, fs["srs"], seed=SEED0 + i, report=how)
        prove_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ok = X.verify(out, fs["compiled"], fs["vk"], fs["srs"])
        verify_s.append(time.perf_counter() - t0)
        if not ok:
            raise SystemExit("leg A: proof %d does not verify" % i)
        hashes.append(hashlib.sha256(proof).hexdigest()[:16])
        paths.append(how.get("path"))
    print(json.dumps(dict(leg="A", tree=TREE, k=meta["k"], proofs=proofs, synthesis_paths=sorted(set(paths)), prove_first_s=round(prove_s[0], 5),
                          prove_rest_s=_spread(prove_s[1:]), verify_first_s=round(verify_s[0], 5), verify_rest_s=_spread(verify_s[1:]), proof_sha256=hashes)))


def leg_b(d, proofs):
    from ezkl_amd import execute as X
    fs, meta = _files(d), json.load(open(_files(d)["meta"]))
    if not hasattr(X, "Prover"):
        print(json.dumps(dict(leg="B", tree=TREE, k=meta["k"], skipped="this tree has no execute.Prover")))
        return
    walls, reports, hashes = [], [], []
    t0 = time.perf_counter()
    with X.Prover(fs["compiled"], fs["pk"], fs["srs"]) as p:
        open_s = time.perf_counter() - t0
        for i in range(proofs):
            wit, out, how = os.path.join(d, "witness%d.json" % (i % meta["n_witnesses"])), os.path.join(d, "proof_b%d.json" % i), {}
            t0 = time.perf_counter()
            proof = p.prove(wit, out, seed=SEED0 + i, report=how)
            walls.append(time.perf_counter() - t0)
            reports.append(how)
            hashes.append(hashlib.sha256(proof).hexdigest()[:16])
        opened = dict(p.opened)
    rest = reports[1:]
    stage_names = sorted({s for r in rest for s in r["stages"]})
    stages = {s: round(statistics.median([r["stages"].get(s, 0.0) for r in rest]), 5) for s in stage_names} if rest else {}
    device_s = statistics.median([r.get("device_ms", 0.0) for r in rest]) / 1e3 if rest else None
    steady = statistics.median(walls[1:]) if rest else None
    print(json.dumps(dict(leg="B", tree=TREE, k=meta["k"], proofs=proofs, synthesis_paths=sorted({r["path"] for r in reports}), open_s=round(open_s, 5),
                          opened={a: round(b, 5) for a, b in opened.items()}, prove_first_s=round(walls[0], 5), prove_rest_s=_spread(walls[1:]),
                          stages_rest_median_s=stages, device_s_rest_median=None if device_s is None else round(device_s, 6),
                          # the share of a steady-state proof that is the plan's replay on the device plus create_proof; everything else is named in stages
                          replay_plus_create_proof_share=None if not rest else round((device_s + stages.get("create_proof", 0.0)) / steady, 4),
                          proof_sha256=hashes)))


def structure(k):
    import pickle
    import struct
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_circuits as BC
    from ezkl_amd import execute as X
    circuit, _ = BC.mlp_circuit(k, np.random.default_rng(1))
    t0 = time.perf_counter(); cs, _, _, reg = X._fresh_keygen_inputs(circuit); t_layout = time.perf_counter() - t0
    bits = np.packbits(np.asarray(reg.selector_rows(), bool), axis=1, bitorder="little").tobytes()
    key = bytes([3, k, 1]) + struct.pack("<I", cs.n_fixed) + bytes(64 * (cs.n_fixed + len(cs.perm))) + bits
    t0 = time.perf_counter(); got = X._plonk_cs(circuit, key); t_key = time.perf_counter() - t0
    print(json.dumps(dict(k=k, layout_s=round(t_layout, 4), from_key_s=round(t_key, 4), n_fixed=[cs.n_fixed, got.n_fixed],
                          gates_equal=pickle.dumps(cs.gates) == pickle.dumps(got.gates), lookups_equal=pickle.dumps(cs.lookups) == pickle.dumps(got.lookups))))


def _child(script, args, seconds, env):
    """one leg, one process, one time limit; -> its last JSON line"""
    cmd = ["timeout", "-k", "10", str(int(seconds)), sys.executable, script] + args
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise SystemExit("%s ended with status %d: nothing more is started" % (" ".join(cmd), r.returncode))
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, action="append")
    ap.add_argument("--proofs", type=int, default=8)
    ap.add_argument("--tag")
    ap.add_argument("--parent", help="a built checkout of the parent commit: this script is copied into its tools/ and its leg A run there, on the same files")
    ap.add_argument("--dir", help="where the artefacts go (default: a temporary directory, removed afterwards)")
    ap.add_argument("--timeout", type=int, default=420, help="seconds for each child process")
    ap.add_argument("--child", choices=["make", "A", "B", "structure"])
    ap.add_argument("--root", help="(with --child) the checkout whose ezkl_amd package the leg imports, instead of this file's own")
    a = ap.parse_args()
    if a.child:
        global TREE
        if a.root:
            sys.path.insert(0, os.path.abspath(a.root))
            TREE = "parent"
            import ezkl_amd
            if not os.path.abspath(ezkl_amd.__file__).startswith(os.path.abspath(a.root) + os.sep):
                raise SystemExit("--root: ezkl_amd was imported from %s" % ezkl_amd.__file__)
        {"structure": lambda: structure(a.k[0]), "make": lambda: make(a.k[0], a.dir, 3), "A": lambda: leg_a(a.dir, a.proofs), "B": lambda: leg_b(a.dir, a.proofs)}[a.child]()
        return
    if not a.k or not a.tag:
        ap.error("--k and --tag are needed")
    env = dict(os.environ, ENABLE_HIP_GPU="1", EZKL_BENCH_CACHE="off")          # the gate open: "auto" makes the witness on the device
    base = a.dir or tempfile.mkdtemp(prefix="prove_files_")
    here = os.path.abspath(__file__)
    out = dict(tag=a.tag, proofs=a.proofs, sizes=[])
    try:
        for k in a.k:
            d = os.path.join(base, "k%d" % k)
            os.makedirs(d, exist_ok=True)
            common = ["--k", str(k), "--dir", d, "--proofs", str(a.proofs)]
            size = dict(k=k, artefacts=_child(here, ["--child", "make"] + common, a.timeout, env))
            if a.parent:
                size["parent_leg_a"] = _child(here, ["--child", "A", "--root", a.parent] + common, a.timeout, env)
            size["leg_a"] = _child(here, ["--child", "A"] + common, a.timeout, env)
            size["leg_b"] = _child(here, ["--child", "B"] + common, a.timeout, env)
            hs = [size[name]["proof_sha256"] for name in ("parent_leg_a", "leg_a", "leg_b") if "proof_sha256" in size.get(name, {})]
            size["proof_bytes_equal_across_legs"] = all(h == hs[0] for h in hs)
            out["sizes"].append(size)
            shutil.rmtree(d, ignore_errors=True)
            path = os.path.join(ROOT, "profiles", a.tag + "_session.json")
            json.dump(out, open(path, "w"), indent=1)
            print("k = %d written to %s" % (k, path), flush=True)
    finally:
        if not a.dir:
            shutil.rmtree(base, ignore_errors=True)
    if not all(s["proof_bytes_equal_across_legs"] for s in out["sizes"]):
        raise SystemExit("proof bytes differ across the legs")


if __name__ == "__main__":
    main()
