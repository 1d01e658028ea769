"""A PoolClassifierCircuit replayed on the device from its recorded plan (csrc/witness.hip) beside the host layout's `synthesize` of the
same inputs -- the witness of every advice cell both ways -- and the arg-extremum kernels alone beside the Python closed form.

    python tools/pool_bench.py --tag <tag>

Circuit legs: the classifier at two sizes -- 8 x 8 image, 3 x 3 kernel, 2 channels, 4 classes at k = 10; 28 x 28 image, 5 x 5 kernel at
stride 2, 4 channels, 10 classes (the conv2d_mnist shapes with a pooling layer and the class decision) at k = 13 -- with max and with sum
pooling, two inner columns.  Per leg the plan is recorded once (record_s); the device leg uploads it and runs it --repeat times after a
first run, timed by HIP events around the whole run (recorded on the stream before the column fills and after the output gather, read
after the stream has drained); the host leg is `PoolClassifierCircuit.synthesize` on the same inputs:

    device_ms        minimum and median of the runs after the first
    host_ms          `synthesize` (the layout engine on Python integers): minimum and median of --host-repeat passes
    records, cells, launches, advice columns

ARGEXT legs: a plan of one INPUT record and one ARGEXT record, segments x length = 1 x 2^10, 1 x 2^18 and 4096 x 10, argmax, values in
+-3 (many ties); the same timing on the device -- so device_ms holds the column fills, the input upload and the INPUT record's launch as
well -- beside `max(range(n), key=lambda j: (s[j], -j))` per segment on Python integers.  The device columns are compared with the host's
byte for byte in every leg.

Every leg runs in a child process of its own under `timeout -k 10`; the driver stops at the first child that does not end clean.  Each
child merges its entry into profiles/<tag>_pool.json."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
W, MAX_ADVICE = 2, 64
LIMIT_S = 300
SIZES = {"small": dict(logrows=10, image=8, kernel=3, out_channels=2, stride=1, classes=4, decomp_legs=3),
         "mnist": dict(logrows=13, image=28, kernel=5, out_channels=4, stride=2, classes=10, decomp_legs=4)}
ARGEXT_SHAPES = [(1, 1 << 10), (1, 1 << 18), (4096, 10)]
LEGS = ["%s-%s" % (size, pool) for size in SIZES for pool in ("max", "sum")] + ["argext-%dx%d" % s for s in ARGEXT_SHAPES]


def classifier(size, pool):
    """-> make(): the circuit with just the blocks its layout needs (one witness-free pass on a configuration with room to spare)"""
    from ezkl_amd import ezkl_layout as EL
    kw = dict(SIZES[size])
    k = kw.pop("logrows")
    roomy = EL.PoolClassifierCircuit(k, W, 9 * W * (1 << k), pool=pool, **kw)
    linear = roomy.synthesize([0] * roomy.n_inputs, witness=False).linear
    make = lambda: EL.PoolClassifierCircuit(k, W, linear + W, pool=pool, **kw)
    assert len(make().gc.cs.advice) <= MAX_ADVICE, "the layout needs more advice columns than a plan may have: raise logrows"
    return make


def timed(dev, x, cols, repeat):
    ms = []
    for i in range(repeat + 1):
        _, outs = dev.run(x, columns=cols)
        if i:                                                                       # the first run after the upload apart
            ms.append(dev.last["device_ms"])
    return outs, dict(min=min(ms), median=float(np.median(ms)))


def circuit_leg(a, B, size, pool):
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    make = classifier(size, pool)
    c = make()
    x = np.random.default_rng(a.seed).integers(0, 16, c.n_inputs).tolist()
    t = time.perf_counter()
    plan = WP.record_plan(make()).validate()
    entry = dict(size=size, pool=pool, k=c.k, inner_cols=W, advice_columns=plan.n_advice, records=int(plan.n_records), cells=int(plan.n_cells),
                 record_s=time.perf_counter() - t)
    host = []
    for _ in range(a.host_repeat):
        t = time.perf_counter()
        reg = c.synthesize(x)
        host.append(1e3 * (time.perf_counter() - t))
    adv, inst = c.witness_of(reg)
    assert [EL.signed(v) for v in inst[0]] == c.model(x)
    dev = B.WitnessPlan(plan.to_bytes())
    cols = dev.alloc_columns()
    try:
        outs, device_ms = timed(dev, x, cols, a.repeat)
        assert dev.last["failed"] == 0 and dev.last["cells_written"] == plan.n_cells and [outs] == inst
        for j, want in enumerate(EL.cols_to_mont(adv, B)):
            assert cols[j].to_numpy(shape=(1 << c.k, 4)).tobytes() == want.tobytes(), "advice column %d of the device is not the host's" % j
        entry.update(launches=dev.last["launches"], device_ms=device_ms, host_ms=dict(min=min(host), median=float(np.median(host))))
    finally:
        for col in cols:
            col.free()
        dev.free()
    return entry


def argext_leg(a, B, segs, n):
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    total = segs * n
    k = max(4, (total - 1).bit_length())
    x = np.random.default_rng(a.seed).integers(-3, 4, total).tolist()
    src, dst = list(range(total)), [(1 << k) + s for s in range(segs)]
    pool = src + list(range(total)) + dst + src                                      # INPUT dst, a; ARGEXT dst, a
    records = [[WP.INPUT, total, 0, 0, 0, total, 0, 0], [WP.ARGEXT, segs, n, 0, 2 * total, 2 * total + segs, 0, 0]]
    plan = WP.WitnessPlan(k, 2, total, [], [], records, dst[:1], pool, total + segs, 2, b"\0" * 32).validate()
    host = []
    for _ in range(a.host_repeat):
        t = time.perf_counter()
        want = [max(range(n), key=lambda j: (x[g * n + j], -j)) for g in range(segs)]
        host.append(1e3 * (time.perf_counter() - t))
    columns = [[v % EL.R for v in x] + [0] * ((1 << k) - total), want + [0] * ((1 << k) - segs)]
    dev = B.WitnessPlan(plan.to_bytes())
    cols = dev.alloc_columns()
    try:
        outs, device_ms = timed(dev, x, cols, a.repeat)
        assert dev.last["failed"] == 0 and dev.last["cells_written"] == plan.n_cells and outs == want[:1]
        for j, col in enumerate(EL.cols_to_mont(columns, B)):
            assert cols[j].to_numpy(shape=(1 << k, 4)).tobytes() == col.tobytes(), "column %d of the device is not the closed form's" % j
        return dict(segments=segs, length=n, k=k, launches=dev.last["launches"], device_ms=device_ms, host_ms=dict(min=min(host), median=float(np.median(host))))
    finally:
        for col in cols:
            col.free()
        dev.free()


def child(a):
    import ezkl_amd
    from ezkl_amd import backend as B
    ezkl_amd.init(0)
    kind, rest = a.leg.split("-", 1)
    entry = argext_leg(a, B, *(int(v) for v in rest.split("x"))) if kind == "argext" else circuit_leg(a, B, kind, rest)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    dst = os.path.join(ROOT, "profiles", "%s_pool.json" % a.tag)
    doc = json.load(open(dst)) if os.path.exists(dst) else {}
    doc[a.leg.replace("-", "_")] = entry
    json.dump(doc, open(dst, "w"), indent=1, sort_keys=True)
    print(json.dumps(entry))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", required=True)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--host-repeat", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--leg", choices=LEGS, default=None, help="one leg, in this process")
    a = ap.parse_args()
    if a.leg is not None:
        return child(a)
    for leg in LEGS:                                                                # one child per leg, each under its own time limit
        cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--tag", a.tag, "--repeat", str(a.repeat), "--host-repeat",
               str(a.host_repeat), "--seed", str(a.seed), "--leg", leg]
        rc = subprocess.call(cmd)
        if rc != 0:
            sys.exit("pool_bench: %s ended with status %d: nothing more is started" % (leg, rc))


if __name__ == "__main__":
    main()
