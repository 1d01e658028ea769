"""A ScatterGatherCircuit replayed on the device from its recorded plan (csrc/witness.hip) beside the host layout's `synthesize` of the same
inputs: the witness of every advice cell both ways.

    python tools/scatter_bench.py --tag <tag>

Legs: the circuit at two sizes, two inner columns -- "small": a 6 x 3 table, a 2 x 3 index and source, 4 picks at k = 10 (the SCATTER and
COMPLEMENT records each run in one workgroup); "tile": a 1400 x 3 table (4200 cells, past SCATTER_TILE = 4096: both records go through the
plan's scratch), a 200 x 3 index and source, 16 picks at k = 15.  Per leg the plan is recorded once (record_s); the device leg uploads it and
runs it --repeat times after a first run, timed by HIP events around the whole run (recorded on the stream before the column fills and after
the output gather, read after the stream has drained); the host leg is `ScatterGatherCircuit.synthesize` on the same inputs:

    device_ms        minimum and median of the runs after the first
    host_ms          `synthesize` (the layout engine on Python integers): minimum and median of --host-repeat passes
    records, cells, launches, advice columns

The device columns are compared with the host's byte for byte in every leg.  Every leg runs in a child process of its own under
`timeout -k 10`; the driver stops at the first child that does not end clean.  Each child merges its entry into profiles/<tag>_scatter.json."""
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
SIZES = {"small": dict(logrows=10, rows=6, cols=3, m=2, picks=4), "tile": dict(logrows=15, rows=1400, cols=3, m=200, picks=16)}
LEGS = list(SIZES)


def circuit(size):
    """-> make(): the circuit with just the blocks its layout needs (one witness-free pass on a configuration with room to spare)"""
    from ezkl_amd import ezkl_layout as EL
    kw = dict(SIZES[size])
    k = kw.pop("logrows")
    roomy = EL.ScatterGatherCircuit(k, W, 9 * W * (1 << k), **kw)
    linear = roomy.synthesize(inputs(roomy, 0), witness=False).linear
    make = lambda: EL.ScatterGatherCircuit(k, W, linear + W, **kw)
    assert len(make().gc.cs.advice) <= MAX_ADVICE, "the layout needs more advice columns than a plan may have: raise logrows"
    return make


def inputs(c, seed):
    """a table, an index with distinct values in every column, a source and the picks"""
    rng = np.random.default_rng(seed)
    index = np.stack([rng.permutation(c.rows)[:c.m] for _ in range(c.cols)], 1).reshape(-1)
    return np.concatenate([rng.integers(-50, 51, c.rows * c.cols), index, rng.integers(-50, 51, c.m * c.cols), rng.integers(0, c.rows, c.picks)]).tolist()


def timed(dev, x, cols, repeat):
    ms = []
    for i in range(repeat + 1):
        _, outs = dev.run(x, columns=cols)
        if i:                                                                       # the first run after the upload apart
            ms.append(dev.last["device_ms"])
    return outs, dict(min=min(ms), median=float(np.median(ms)))


def leg(a, B, size):
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    make = circuit(size)
    c = make()
    x = inputs(c, a.seed)
    t = time.perf_counter()
    plan = WP.record_plan(make()).validate()
    kinds = plan.records[:, 0].tolist()
    entry = dict(size=size, k=c.k, inner_cols=W, table=[c.rows, c.cols], elements=c.m * c.cols, picks=c.picks, scatter_tile=WP.SCATTER_TILE, advice_columns=plan.n_advice,
                 records=int(plan.n_records), cells=int(plan.n_cells), record_s=time.perf_counter() - t)
    assert (kinds.count(WP.SCATTER), kinds.count(WP.COMPLEMENT), kinds.count(WP.ONEHOT)) == (1, 1, 1)
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


def child(a):
    import ezkl_amd
    from ezkl_amd import backend as B
    ezkl_amd.init(0)
    entry = leg(a, B, a.leg)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    dst = os.path.join(ROOT, "profiles", "%s_scatter.json" % a.tag)
    doc = json.load(open(dst)) if os.path.exists(dst) else {}
    doc[a.leg] = entry
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
    for name in LEGS:                                                               # one child per leg, each under its own time limit
        cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--tag", a.tag, "--repeat", str(a.repeat), "--host-repeat",
               str(a.host_repeat), "--seed", str(a.seed), "--leg", name]
        rc = subprocess.call(cmd)
        if rc != 0:
            sys.exit("scatter_bench: %s ended with status %d: nothing more is started" % (name, rc))


if __name__ == "__main__":
    main()
