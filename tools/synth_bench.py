"""Witness synthesis of the bench MLP (tools/bench_circuits.py kind="mlp"; --circuit conv: its kind="conv", ConvMnistCircuit(logrows=k) on
the bench's image distribution): the host path against the device path, per circuit size.

    host_s          circuit.witness(x) + cols_to_mont -- what `execute.prove(synthesis="host")` does before create_proof: the yardstick
    record_plan_s   witness_plan.record_plan -- a SETUP cost (once per circuit, `execute.setup` writes the plan next to the key)
    device_ms       one synthesis on the device, HIP events around the run (fills, input upload, one launch per record, output gather):
                    the first run after the upload apart, then the minimum and median of --repeat runs
    plan_bytes, records, launches, cells

One process per size, every GPU step under its own time limit:

    timeout -k 10 600 python tools/synth_bench.py --k 14 --tag <tag> && timeout -k 10 900 python tools/synth_bench.py --k 17 --tag <tag>

--circuit einsum: the bench's EinsumMatmulCircuit (tools/bench_circuits.py kind="einsum": len 64 / 180 / 512 at k = 14 / 17 / 20), whose
second-phase columns depend on the proof's challenges, so the host pass runs INSIDE create_proof, once per phase:

    host_s              both phases of circuit.advice_fn + cols_to_mont -- what the per-phase callback of create_proof costs: the yardstick
    device_phase0/1_*   the phase-0 run and the phase-1 run of the plan, HIP events around each: first run, minimum and median of --repeat
    create_proof_*_s    wall time of native.create_proof with the host callable and with the device callable (backend.WitnessPlan.advice_fn),
                        same key and seed; the proof bytes must be equal (--skip-proof leaves the pair out)

--rebase D (MLP): every Gemm of the bench MLP wrapped in the RebaseScale division by D (layouts.rs:219-267 `div`, ezkl_layout.BaseRegion.div):
the circuit ezkl lays out at non-zero scales; its entry is keyed "k<k>_rebase<D>".

--circuit transformer: the bench's TransformerSurrogateCircuit (tools/bench_circuits.py kind="transformer"), the one circuit that is TILED: the host
path lays one unit out in Python, tiles it with numpy, converts and uploads every column -- phase 0 once, phase 1 inside create_proof for every
proof --, the device path replays the circuit's two-phase plan and tiles on the device (build(synthesis="device")):

    host_unit_layout_s  one Python pass of the unit (BaseRegion + `layout`): part of what build() does before anything else
    host_phase0/1_s     build()'s advice(0, []) / advice(1, challenges), uncached -- phase 1 is the Freivalds pass, the tile and the Montgomery
                        conversion of three columns --, each followed by the upload of its columns (host_phase*_upload_s, included): the yardstick
    device_phase0/1_*   HIP events of the plan's run and of the tile launch of that phase: first call, minimum and median of --repeat
    create_proof_*_s    wall time of native.create_proof with the host callable and with the device callable on one key and seed; the bytes are compared

Each run merges its entry into profiles/<tag>_synth.json (key "k<k>" for the MLP, "conv_k<k>" for --circuit conv, "einsum_k<k>", "transformer_k<k>").  --skip-host leaves the host pass out (k = 20: over a minute of Python);
--plan-dir keeps recorded plans between runs (a plan depends only on the circuit)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, required=True)
    ap.add_argument("--circuit", choices=("mlp", "conv", "einsum", "transformer"), default="mlp")
    ap.add_argument("--skip-proof", action="store_true", help="einsum: leave the create_proof pair out")
    ap.add_argument("--tag", default="synth")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--base", type=int, default=None, help="decomposition base (default: the bench's 16384)")
    ap.add_argument("--rebase", type=int, default=None, help="mlp: wrap every Gemm in the RebaseScale division by this integer (key \"k<k>_rebase<d>\")")
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--plan-dir", default=None)
    a = ap.parse_args()
    import bench_circuits as BC
    import ezkl_amd
    from ezkl_amd import backend as B, ezkl_layout as EL, witness_plan as WP
    ezkl_amd.init()
    if a.circuit == "einsum":
        return einsum(a)
    if a.circuit == "transformer":
        return transformer(a)
    if a.circuit == "conv":
        circuit = EL.ConvMnistCircuit(logrows=a.k, seed=a.seed)
        img = np.random.default_rng(a.seed).integers(0, 16, (28, 28))        # MNIST pixels / 16, as tools/bench_circuits.py kind="conv" draws them
        x, witness_in = [int(v) for v in img.reshape(-1)], img
        what = "examples/conv2d_mnist: Conv 1->4 5x5 stride 2 on 28x28 + ReLU + Div{32} lookup + Linear 576->10"
    else:
        circuit, x = BC.mlp_circuit(a.k, np.random.default_rng(a.seed), base=a.base, rebase=a.rebase)
        witness_in = x
        what = "MLP %d x (Gemm %dx%d%s + bias + ReLU), base %d" % (len(circuit.weights), len(circuit.weights[0]), len(circuit.weights[0]),
                                                                  " / %d" % a.rebase if a.rebase else "", circuit.base)
    out = dict(k=a.k, circuit=what, advice_columns=len(circuit.gc.cs.advice))
    host = None
    if not a.skip_host:
        t = time.perf_counter()
        adv, inst = circuit.witness(witness_in)
        t1 = time.perf_counter()
        host = EL.cols_to_mont(adv, B)
        B.synchronize()
        t2 = time.perf_counter()
        out.update(host_witness_s=round(t1 - t, 3), host_cols_to_mont_s=round(t2 - t1, 3), host_s=round(t2 - t, 3))
        print("k=%d host: circuit.witness %.3f s + cols_to_mont %.3f s" % (a.k, t1 - t, t2 - t1), flush=True)
    blob, path = None, a.plan_dir and os.path.join(a.plan_dir, "%s_k%d_s%d_b%d%s.wplan" % (a.circuit, a.k, a.seed, circuit.base, "_r%d" % a.rebase if a.rebase else ""))
    if path and os.path.exists(path):
        blob = open(path, "rb").read()
        if WP.peek(blob)["param_hash"] != WP.params_hash(circuit):
            blob = None
    if blob is None:
        t = time.perf_counter()
        plan = WP.record_plan(circuit)
        out["record_plan_s"] = round(time.perf_counter() - t, 3)
        print("k=%d plan recording (setup, once per circuit): %.3f s" % (a.k, out["record_plan_s"]), flush=True)
        blob = plan.to_bytes()
        if path:
            os.makedirs(a.plan_dir, exist_ok=True)
            open(path, "wb").write(blob)
    h = WP.peek(blob)
    t = time.perf_counter()
    dev = B.WitnessPlan(blob)
    out.update(plan_bytes=len(blob), records=h["n_records"], layout_ops=h["n_ops"], cells=h["n_cells"], plan_upload_s=round(time.perf_counter() - t, 3))
    cols = dev.alloc_columns()
    _, outs = dev.run(x, columns=cols)
    out.update(launches=dev.last["launches"], cells_written=dev.last["cells_written"], device_first_ms=round(dev.last["device_ms"], 4))
    assert dev.last["cells_written"] == h["n_cells"]
    if host is not None:                             # the run that is timed computes what the host computes
        n = 1 << a.k
        assert [outs] == inst
        for c, r in zip(cols, host):
            assert c.to_numpy(shape=(n, 4)).tobytes() == np.ascontiguousarray(r).tobytes()
        out["columns_equal_host"] = True
    ms, wall = [], []
    for _ in range(a.repeat):
        t = time.perf_counter()
        dev.run(x, columns=cols)
        wall.append((time.perf_counter() - t) * 1e3)
        ms.append(dev.last["device_ms"])
    out.update(device_ms_min=round(min(ms), 4), device_ms_median=round(float(np.median(ms)), 4), device_call_wall_ms_median=round(float(np.median(wall)), 4),
               repeat=a.repeat)
    print("k=%d device: %.3f ms min, %.3f ms median of %d (first %.3f ms); %d launches for %d records / %d layout ops; plan %d bytes, %d cells"
          % (a.k, min(ms), float(np.median(ms)), a.repeat, out["device_first_ms"], out["launches"], out["records"], out["layout_ops"], len(blob), h["n_cells"]), flush=True)
    for c in cols:
        c.free()
    dev.free()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    dst = os.path.join(ROOT, "profiles", "%s_synth.json" % a.tag)
    doc = json.load(open(dst)) if os.path.exists(dst) else {}
    doc[("k%d" if a.circuit == "mlp" else "conv_k%d") % a.k + ("_rebase%d" % a.rebase if a.rebase and a.circuit == "mlp" else "")] = out
    json.dump(doc, open(dst, "w"), indent=1, sort_keys=True)
    print(json.dumps(out))


EINSUM_LEN = {20: 512, 17: 180, 14: 64, 12: 30, 10: 14}
EINSUM_CHALLENGES = [0x1234567890abcdef1234567890abcdef1234567890abcdef1234567890abcdef, 0x0fedcba0987654321fedcba0987654321fedcba0987654321fedcba098765432]


def einsum(a):
    from ezkl_amd import backend as B, ezkl_layout as EL, native as NV, witness_plan as WP
    k, L = a.k, EINSUM_LEN[a.k]
    n = 1 << k
    circuit = EL.EinsumMatmulCircuit(k, L)
    rng = np.random.default_rng(a.seed)
    ma, mb = rng.integers(-128, 128, (L, L)), rng.integers(-128, 128, (L, L))        # as tools/bench_circuits.py kind="einsum" draws them
    x = [int(v) for v in ma.reshape(-1)] + [int(v) for v in mb.reshape(-1)]
    n_adv = len(circuit.cs.advice)
    chal = [c % EL.R for c in EINSUM_CHALLENGES]
    out = dict(k=k, circuit="accum_einsum_matmul ij,jk->ik len %d, Freivalds" % L, advice_columns=n_adv)
    fn = circuit.advice_fn(ma, mb, n_adv)
    def host_fn(phase, challenges):
        cols = fn(phase, challenges)
        idx = sorted(cols)
        return dict(zip(idx, EL.cols_to_mont([cols[i] for i in idx], B)))
    host = None
    if not a.skip_host:
        t = time.perf_counter()
        p0 = fn(0, [])
        t1 = time.perf_counter()
        p1 = fn(1, chal)
        t2 = time.perf_counter()
        cols = {**p0, **p1}
        host = EL.cols_to_mont([cols[i] for i in range(n_adv)], B)
        B.synchronize()
        t3 = time.perf_counter()
        out.update(host_phase0_s=round(t1 - t, 3), host_phase1_s=round(t2 - t1, 3), host_cols_to_mont_s=round(t3 - t2, 3), host_s=round(t3 - t, 3))
        print("k=%d host: advice_fn phase 0 %.3f s + phase 1 %.3f s + cols_to_mont %.3f s" % (k, t1 - t, t2 - t1, t3 - t2), flush=True)
    t = time.perf_counter()
    plan = WP.record_plan(circuit)
    out["record_plan_s"] = round(time.perf_counter() - t, 3)
    blob = plan.to_bytes()
    t = time.perf_counter()
    dev = B.WitnessPlan(blob)
    out.update(plan_bytes=len(blob), records=plan.n_records, cells=plan.n_cells, plan_upload_s=round(time.perf_counter() - t, 3))
    cols = dev.alloc_columns()
    ms = {0: [], 1: []}
    launches = written = 0
    for it in range(a.repeat + 1):
        for phase in (0, 1):
            dev.run(x, columns=cols, phase=phase, challenges=chal if phase else ())
            ms[phase].append(dev.last["device_ms"])
            if it == 0:
                launches += dev.last["launches"]
                written += dev.last["cells_written"]
        if it == 0:
            assert written == plan.n_cells
            if host is not None:                 # the run that is timed computes what the host computes
                for c, r in zip(cols, host):
                    assert c.to_numpy(shape=(n, 4)).tobytes() == np.ascontiguousarray(r).tobytes()
                out["columns_equal_host"] = True
    for phase in (0, 1):
        out.update({"device_phase%d_first_ms" % phase: round(ms[phase][0], 4), "device_phase%d_ms_min" % phase: round(min(ms[phase][1:]), 4),
                    "device_phase%d_ms_median" % phase: round(float(np.median(ms[phase][1:])), 4)})
    out.update(launches=launches, cells_written=written, repeat=a.repeat,
               device_ms_min=round(min(ms[0][1:]) + min(ms[1][1:]), 4), device_ms_median=round(float(np.median(ms[0][1:]) + np.median(ms[1][1:])), 4))
    print("k=%d device: phase 0 %.3f ms + phase 1 %.3f ms (median of %d; first %.3f + %.3f ms); %d launches for %d records; plan %d bytes, %d cells"
          % (k, out["device_phase0_ms_median"], out["device_phase1_ms_median"], a.repeat, ms[0][0], ms[1][0], launches, plan.n_records, len(blob), plan.n_cells), flush=True)
    if not a.skip_proof:
        t = time.perf_counter()
        cs, fixed, copies, rows = circuit.keygen_inputs(ma, mb)
        bg, bgl = B.gen_srs(k, 0x5eed)
        pk = NV.NativeProvingKey(NV.NativeCircuit(cs), bg, EL.cols_to_mont(fixed, B), copies)
        out["keygen_s"] = round(time.perf_counter() - t, 3)
        NV.create_proof(pk, bg, bgl, dev.advice_fn(x, cols), seed=7, device_columns=range(n_adv))          # warm: the sweep kernel, the tables
        t = time.perf_counter()
        got = NV.create_proof(pk, bg, bgl, dev.advice_fn(x, cols), seed=7, device_columns=range(n_adv))
        out["create_proof_device_s"] = round(time.perf_counter() - t, 4)
        out["create_proof_device_witness_ms"] = round(sum(dev.phase_ms.values()), 4)
        if not a.skip_host:
            t = time.perf_counter()
            ref = NV.create_proof(pk, bg, bgl, host_fn, seed=7)
            out["create_proof_host_s"] = round(time.perf_counter() - t, 4)
            assert got == ref, "the proof from the device callable differs from the host callable's"
            out["proof_bytes_equal"] = True
        print("k=%d create_proof: device callable %.4f s%s" % (k, out["create_proof_device_s"],
              ", host callable %.4f s, same bytes" % out["create_proof_host_s"] if "create_proof_host_s" in out else ""), flush=True)
        bg.free(); bgl.free()
    for c in cols:
        c.free()
    dev.free()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    dst = os.path.join(ROOT, "profiles", "%s_synth.json" % a.tag)
    doc = json.load(open(dst)) if os.path.exists(dst) else {}
    doc["einsum_k%d" % k] = out
    json.dump(doc, open(dst, "w"), indent=1, sort_keys=True)
    print(json.dumps(out))


def transformer(a):
    from ezkl_amd import backend as B, ezkl_layout as EL, native as NV
    k = a.k
    n = 1 << k
    small = k < 16                                    # as tools/bench_circuits.py kind="transformer" shapes it
    make = lambda: EL.TransformerSurrogateCircuit(k, blocks=4, d=4 if small else 64, einsum_len=3 if small else 48, decomp_base=a.base or (16 if small else 16384),
                                                  lookup_max=(1 << k) // 16 if small else None, seed=a.seed)
    chal = [c % EL.R for c in EINSUM_CHALLENGES]
    c = make()
    t = time.perf_counter()
    reg = EL.BaseRegion(c.gc, True)
    c.layout(reg, [EL.Val(v) for v in c.default_inputs()], EL.Val)
    out = dict(k=k, host_unit_layout_s=round(time.perf_counter() - t, 4))
    t = time.perf_counter()
    host = make().build(gpu=B)
    out["host_build_s"] = round(time.perf_counter() - t, 3)
    n_adv = host["cs"].n_advice
    out.update(circuit=host["info"]["circuit"], advice_columns=n_adv, unit_rows=host["info"]["unit_rows"], tiles=host["info"]["tiles"], blocks=host["info"]["blocks"])
    host_cols = {}
    for phase in (0, 1):                              # the host callable as create_proof calls it, then the upload create_proof makes of what it returns
        B.synchronize()
        t = time.perf_counter()
        cols = host["advice"](phase, chal if phase else [])
        t1 = time.perf_counter()
        up = [B.DeviceBuffer.from_numpy(cols[i]) for i in sorted(cols)]
        B.synchronize()
        t2 = time.perf_counter()
        for u in up:
            u.free()
        host_cols.update(cols)
        out.update({"host_phase%d_s" % phase: round(t2 - t, 4), "host_phase%d_upload_s" % phase: round(t2 - t1, 4), "host_phase%d_columns" % phase: len(cols)})
    out["host_s"] = round(out["host_phase0_s"] + out["host_phase1_s"], 4)
    print("k=%d host: unit layout %.3f s, build %.3f s; advice(0) %.3f s (upload %.3f s) + advice(1) %.3f s (upload %.3f s)"
          % (k, out["host_unit_layout_s"], out["host_build_s"], out["host_phase0_s"], out["host_phase0_upload_s"], out["host_phase1_s"], out["host_phase1_upload_s"]), flush=True)
    t = time.perf_counter()
    dev = make().build(gpu=B, synthesis="device")
    out["device_build_s"] = round(time.perf_counter() - t, 3)
    w = dev["witness"]
    out.update(records=w.plan.n_records, cells=w.plan.n_cells, tile_pairs=[len(w.pairs[0]), len(w.pairs[1])])
    ms = {(p, what): [] for p in (0, 1) for what in ("run", "tile")}
    for it in range(a.repeat + 1):
        got = {}
        for phase in (0, 1):
            got.update(dev["advice"](phase, chal if phase else []))
            ms[(phase, "run")].append(w.phase_ms[phase][0])
            ms[(phase, "tile")].append(w.phase_ms[phase][1])
        if it == 0:                                   # the run that is timed computes what the host computes
            for i in range(n_adv):
                assert got[i].to_numpy(shape=(n, 4)).tobytes() == np.ascontiguousarray(host_cols[i]).tobytes(), "advice column %d differs from the host callable's" % i
            out["columns_equal_host"] = True
    for (phase, what), v in ms.items():
        out.update({"device_phase%d_%s_first_ms" % (phase, what): round(v[0], 4), "device_phase%d_%s_ms_min" % (phase, what): round(min(v[1:]), 4),
                    "device_phase%d_%s_ms_median" % (phase, what): round(float(np.median(v[1:])), 4)})
    out.update(repeat=a.repeat, device_ms_median=round(sum(float(np.median(v[1:])) for v in ms.values()), 4), device_ms_min=round(sum(min(v[1:]) for v in ms.values()), 4))
    print("k=%d device (median of %d): phase 0 run %.3f + tile %.3f ms, phase 1 run %.3f + tile %.3f ms; %d records, unit %d rows x %d tiles x %d blocks"
          % (k, a.repeat, *[out["device_phase%d_%s_ms_median" % pw] for pw in ((0, "run"), (0, "tile"), (1, "run"), (1, "tile"))], w.plan.n_records,
             out["unit_rows"], out["tiles"], out["blocks"]), flush=True)
    if not a.skip_proof:
        t = time.perf_counter()
        bg, bgl = B.gen_srs(k, 0x5eed)
        pk = NV.NativeProvingKey(NV.NativeCircuit(host["cs"]), bg, EL.cols_to_mont(host["fixed"], B), host["copies"])
        out["keygen_s"] = round(time.perf_counter() - t, 3)
        prove_dev = lambda: NV.create_proof(pk, bg, bgl, dev["advice"], seed=7, instances=dev["instances"], device_columns=dev["device_columns"])
        prove_dev()                                   # warm: the sweep kernel, the tables
        t = time.perf_counter()
        got = prove_dev()
        out["create_proof_device_s"] = round(time.perf_counter() - t, 4)
        out["create_proof_device_witness_ms"] = round(sum(sum(v) for v in w.phase_ms.values()), 4)
        fresh = make().build(gpu=B)                   # an advice callable with nothing cached: what a proof of new inputs pays
        t = time.perf_counter()
        ref = NV.create_proof(pk, bg, bgl, fresh["advice"], seed=7, instances=fresh["instances"])
        out["create_proof_host_s"] = round(time.perf_counter() - t, 4)
        t = time.perf_counter()
        again = NV.create_proof(pk, bg, bgl, fresh["advice"], seed=7, instances=fresh["instances"])
        out["create_proof_host_cached_s"] = round(time.perf_counter() - t, 4)      # the same challenges again: the callable answers from its cache
        assert got == ref == again, "the proof from the device callable differs from the host callable's"
        out["proof_bytes_equal"] = True
        print("k=%d create_proof: device callable %.4f s, host callable %.4f s (its cache warm: %.4f s), same bytes"
              % (k, out["create_proof_device_s"], out["create_proof_host_s"], out["create_proof_host_cached_s"]), flush=True)
        bg.free(); bgl.free()
    w.free()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    dst = os.path.join(ROOT, "profiles", "%s_synth.json" % a.tag)
    doc = json.load(open(dst)) if os.path.exists(dst) else {}
    doc["transformer_k%d" % k] = out
    json.dump(doc, open(dst, "w"), indent=1, sort_keys=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
