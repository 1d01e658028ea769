"""A softmax over the rows of a NormCircuit replayed on the device from its recorded plan (csrc/witness.hip) beside the host layout's
`synthesize` of the same inputs -- the witness of every advice cell both ways.

    python tools/norm_bench.py --tag <tag>

Shapes at k = 14, two inner columns: 64 rows x 64, and the most rows of 64 whose layout fits the 64 advice columns a plan may have.  Per
shape the plan is recorded once (record_s); the device leg uploads it and runs it --repeat times after a first run, timed by HIP events
around the whole run (host and device around each other: the events are recorded on the stream before the column fills and after the
output gather, and read after the stream has drained); the host leg is `NormCircuit.synthesize` on the same inputs:

    device_ms        minimum and median of the runs after the first
    host_ms          `synthesize` (the layout engine on Python integers): minimum and median of --host-repeat passes
    records, cells, launches, advice columns

Every shape runs in a child process of its own under `timeout -k 10`; the driver stops at the first child that does not end clean.  Each
child merges its entry into profiles/<tag>_norm.json."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
K, W, LENGTH, MAX_ADVICE = 14, 2, 64, 64
LIMIT_S = 420


def cells_needed(rows, length):
    """the linear coordinate a layout of rows x length ends at: one witness-free pass on a configuration with room to spare"""
    from ezkl_amd import ezkl_layout as EL
    c = EL.NormCircuit(K, W, 9 * W * (1 << K), rows, length)
    return c.synthesize([0] * (rows * length), witness=False).linear


def largest_rows(length):
    """the most rows whose layout fits (MAX_ADVICE - 3) // 3 // W blocks of W columns of 2^K rows: the cost is one row's, row after row"""
    one, two = cells_needed(1, length), cells_needed(2, length)
    blocks = (MAX_ADVICE - 3) // 3 // W
    room = blocks * W * ((1 << K) - 64)                                             # rows of a column that are certainly usable
    return (room - one) // (two - one) + 1, blocks


def child(a):
    import ezkl_amd
    from ezkl_amd import backend as B, ezkl_layout as EL, witness_plan as WP
    rows, length = a.shape
    _, blocks = largest_rows(length)
    capacity = blocks * W * ((1 << K) - 64)
    make = lambda: EL.NormCircuit(K, W, capacity, rows, length)
    x = np.random.default_rng(a.seed).integers(-12, 13, rows * length).tolist()
    t = time.perf_counter()
    plan = WP.record_plan(make()).validate()
    entry = dict(rows=rows, length=length, k=K, inner_cols=W, advice_columns=plan.n_advice, records=int(plan.n_records), cells=int(plan.n_cells),
                 record_s=time.perf_counter() - t)
    host, c = [], make()
    for _ in range(a.host_repeat):
        t = time.perf_counter()
        reg = c.synthesize(x)
        host.append(1e3 * (time.perf_counter() - t))
    adv, inst = c.witness_of(reg)
    ezkl_amd.init(0)
    dev = B.WitnessPlan(plan.to_bytes())
    cols = dev.alloc_columns()
    try:
        ms = []
        for i in range(a.repeat + 1):
            _, outs = dev.run(x, columns=cols)
            if i:                                                                   # the first run after the upload apart
                ms.append(dev.last["device_ms"])
        assert dev.last["failed"] == 0 and dev.last["cells_written"] == plan.n_cells and [outs] == inst
        n = 1 << K
        for j, want in enumerate(EL.cols_to_mont(adv, B)):
            assert cols[j].to_numpy(shape=(n, 4)).tobytes() == want.tobytes(), "advice column %d of the device is not the host's" % j
        entry.update(launches=dev.last["launches"], device_ms=dict(min=min(ms), median=float(np.median(ms))),
                     host_ms=dict(min=min(host), median=float(np.median(host))))
    finally:
        for col in cols:
            col.free()
        dev.free()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    dst = os.path.join(ROOT, "profiles", "%s_norm.json" % a.tag)
    doc = json.load(open(dst)) if os.path.exists(dst) else {}
    doc["softmax_%dx%d" % (rows, length)] = entry
    json.dump(doc, open(dst, "w"), indent=1, sort_keys=True)
    print(json.dumps(entry))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", required=True)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--host-repeat", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--shape", type=lambda s: tuple(int(v) for v in s.split("x")), default=None, help="rows x length: one shape, in this process")
    a = ap.parse_args()
    if a.shape is not None:
        return child(a)
    most, _ = largest_rows(LENGTH)
    for rows in (64, most):                                                         # one child per shape, each under its own time limit
        cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--tag", a.tag, "--repeat", str(a.repeat), "--host-repeat",
               str(a.host_repeat), "--seed", str(a.seed), "--shape", "%dx%d" % (rows, LENGTH)]
        rc = subprocess.call(cmd)
        if rc != 0:
            sys.exit("norm_bench: %d x %d ended with status %d: nothing more is started" % (rows, LENGTH, rc))


if __name__ == "__main__":
    main()
