#!/usr/bin/env python3
"""What the visibilities of the MLP family cost on artefact files, next to the default triple of the SAME model in the same sitting.

    python tools/visibility_bench.py --k 14 --k 17 --proofs 6 --tag TAG [--parent DIR] [--dir DIR] [--timeout SECONDS]

The circuit is the bench MLP (tools/bench_circuits.mlp_circuit) written as this package's JSON description, once per variant:
    default     Private / Private / Public          public_in   Public / Private / Public
    fixed       Private / Fixed / Public            committed   KZGCommit / KZGCommit / KZGCommit
For each variant, in a process of its own under its own `timeout -k 10`: the artefacts (execute.gen_srs once per size, setup per variant;
their wall is recorded, not compared), then `gen_witness` on the host and on the device (median of --repeats calls, the SRS given so that
a committed tensor is committed), a resident `execute.Prover` session of --proofs proofs (first, then median and minimum of the rest)
and `verify`.  For the committed variant the seconds spent inside backend.polycommit_commit (host path: the message as integers) and
backend.polycommit_commit_dev (device path: the replayed columns) are recorded too: what the device-side commitment saves.
--parent DIR (a built checkout of the parent commit) measures the default variant with THAT checkout's package on the same files, before
and after this tree's own run of it: the default triple's code path must not have moved, and the two parent runs give the spread.
A child that fails ends the run.  Result: profiles/<tag>_visibility.json."""
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
SEED0 = 7
VARIANTS = {"default": ("Private", "Private", "Public"), "public_in": ("Public", "Private", "Public"), "fixed": ("Private", "Fixed", "Public"),
            "committed": ("KZGCommit", "KZGCommit", "KZGCommit")}


def _files(d, variant):
    f = lambda name: os.path.join(d, variant + "_" + name)
    return dict(compiled=f("model.json"), vk=f("vk.key"), pk=f("pk.key"), data=os.path.join(d, "input.json"), srs=os.path.join(d, "kzg.srs"))


def make(k, d, variant):
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_circuits as BC
    from ezkl_amd import execute as X
    circuit, x = BC.mlp_circuit(k, np.random.default_rng(1))
    fs, t, tri = _files(d, variant), {}, VARIANTS[variant]
    ra = dict(logrows=k, num_inner_cols=circuit.w, decomp_base=circuit.base, decomp_legs=circuit.legs)
    if variant != "default":                             # the default description is the one every revision of the package reads
        ra.update(input_visibility=tri[0], param_visibility=tri[1], output_visibility=tri[2])
    json.dump({"model": "mlp", "run_args": ra, "weights": circuit.weights, "biases": circuit.biases, "total_assignments": circuit.settings.total_assignments},
              open(fs["compiled"], "w"))
    json.dump({"input_data": [[float(v) for v in x]]}, open(fs["data"], "w"))
    if not os.path.exists(fs["srs"]):
        t0 = time.time(); X.gen_srs(fs["srs"], k, secret=0x5eed); t["gen_srs"] = round(time.time() - t0, 3)
    t0 = time.time(); info = X.setup(fs["compiled"], fs["srs"], fs["vk"], fs["pk"]); t["setup"] = round(time.time() - t0, 3)
    print(json.dumps(dict(variant=variant, k=k, seconds=t, setup=info, parameters=sum(len(W) * len(W[0]) + len(W) for W in circuit.weights),
                          bytes=dict(pk=os.path.getsize(fs["pk"]), wplan=os.path.getsize(fs["pk"] + ".wplan")))))


def _spread(xs):
    return dict(median=round(statistics.median(xs), 5), min=round(min(xs), 5), max=round(max(xs), 5), n=len(xs)) if xs else None


def run(k, d, variant, proofs, repeats, tree):
    from ezkl_amd import backend as B, execute as X
    fs = _files(d, variant)
    inside = {}
    def timed(name):
        f = getattr(B, name, None)
        if f is None:
            return
        def g(*a, **kw):
            t0 = time.perf_counter()
            try:
                return f(*a, **kw)
            finally:
                inside[name] = inside.get(name, 0.0) + time.perf_counter() - t0
        setattr(B, name, g)
    timed("polycommit_commit"); timed("polycommit_commit_dev")
    out = dict(variant=variant, tree=tree, k=k)
    texts = {}
    for how in ("host", "device"):
        walls = []
        for i in range(repeats + 1):                     # the first call of each path is reported apart: it loads the library's kernels
            inside.clear()
            wit = os.path.join(d, "%s_%s_witness_%s.json" % (variant, tree, how))
            t0 = time.perf_counter()
            X.gen_witness(fs["compiled"], fs["data"], output=wit, vk_path=fs["vk"], srs_path=fs["srs"], synthesis=how, pk_path=fs["pk"])
            walls.append(time.perf_counter() - t0)
        texts[how] = open(wit, "rb").read()
        out["gen_witness_%s_first_s" % how], out["gen_witness_%s_s" % how] = round(walls[0], 5), _spread(walls[1:])
        out["gen_witness_%s_commit_inside_s" % how] = {a: round(b, 5) for a, b in inside.items()}
    out["witness_files_equal"] = texts["host"] == texts["device"]
    walls, verify_s, reports = [], [], []
    t0 = time.perf_counter()
    with X.Prover(fs["compiled"], fs["pk"], fs["srs"]) as p:
        out["open_s"] = round(time.perf_counter() - t0, 5)
        for i in range(proofs):
            how, path = {}, os.path.join(d, "%s_%s_proof.json" % (variant, tree))
            t0 = time.perf_counter()
            p.prove(wit, path, seed=SEED0 + i, report=how)
            walls.append(time.perf_counter() - t0)
            reports.append(how)
            t0 = time.perf_counter()
            if not X.verify(path, fs["compiled"], fs["vk"], fs["srs"]):
                raise SystemExit("%s: proof %d does not verify" % (variant, i))
            verify_s.append(time.perf_counter() - t0)
    rest = reports[1:]
    out.update(synthesis_paths=sorted({r["path"] for r in reports}), prove_first_s=round(walls[0], 5), prove_rest_s=_spread(walls[1:]),
               verify_rest_s=_spread(verify_s[1:]), proof_bytes=os.path.getsize(path),
               replay_device_ms=_spread([r.get("device_ms", 0.0) for r in rest]),
               create_proof_s=_spread([r["stages"]["create_proof"] for r in rest]))
    print(json.dumps(out))


def _child(args, seconds, env):
    """one step, one process, one time limit; -> its last JSON line"""
    cmd = ["timeout", "-k", "10", str(int(seconds)), sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise SystemExit("%s ended with status %d: nothing more is started" % (" ".join(cmd), r.returncode))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, action="append")
    ap.add_argument("--proofs", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--variant", action="append", choices=list(VARIANTS))
    ap.add_argument("--tag")
    ap.add_argument("--parent", help="a built checkout of the parent commit: the default variant is measured with its package too, on the same files")
    ap.add_argument("--dir", help="where the artefacts go (default: a temporary directory, removed afterwards)")
    ap.add_argument("--timeout", type=int, default=420, help="seconds for each child process")
    ap.add_argument("--child", choices=["make", "run"])
    ap.add_argument("--root", help="(with --child) the checkout whose ezkl_amd package the step imports, instead of this file's own")
    a = ap.parse_args()
    if a.child:
        tree = "this"
        if a.root:
            sys.path.insert(0, os.path.abspath(a.root))
            tree = "parent"
            import ezkl_amd
            if not os.path.abspath(ezkl_amd.__file__).startswith(os.path.abspath(a.root) + os.sep):
                raise SystemExit("--root: ezkl_amd was imported from %s" % ezkl_amd.__file__)
        if a.child == "make":
            make(a.k[0], a.dir, a.variant[0])
        else:
            run(a.k[0], a.dir, a.variant[0], a.proofs, a.repeats, tree)
        return
    if not a.k or not a.tag:
        ap.error("--k and --tag are needed")
    env = dict(os.environ, ENABLE_HIP_GPU="1", EZKL_BENCH_CACHE="off")          # the gate open: "auto" makes the witness on the device
    base = a.dir or tempfile.mkdtemp(prefix="visibility_")
    out = dict(tag=a.tag, proofs=a.proofs, repeats=a.repeats, sizes=[])
    path = os.path.join(ROOT, "profiles", a.tag + "_visibility.json")
    try:
        for k in a.k:
            d = os.path.join(base, "k%d" % k)
            os.makedirs(d, exist_ok=True)
            size = dict(k=k, variants={})
            out["sizes"].append(size)
            for variant in a.variant or list(VARIANTS):
                common = ["--k", str(k), "--dir", d, "--variant", variant, "--proofs", str(a.proofs), "--repeats", str(a.repeats)]
                v = size["variants"][variant] = dict(artefacts=_child(["--child", "make"] + common, a.timeout, env))
                if a.parent and variant == "default":
                    v["parent_before"] = _child(["--child", "run", "--root", a.parent] + common, a.timeout, env)
                v["run"] = _child(["--child", "run"] + common, a.timeout, env)
                if a.parent and variant == "default":
                    v["parent_after"] = _child(["--child", "run", "--root", a.parent] + common, a.timeout, env)
                json.dump(out, open(path, "w"), indent=1)
                print("k = %d %s written to %s" % (k, variant, path), flush=True)
            shutil.rmtree(d, ignore_errors=True)
    finally:
        if not a.dir:
            shutil.rmtree(base, ignore_errors=True)


if __name__ == "__main__":
    main()
