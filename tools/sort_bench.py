"""One SORT + ARGSORT pair of a witness plan on the device (csrc/witness.hip) beside np.lexsort of the same keys on the host -- what a host
layout would pay for the data-dependent step at best, before it places a single cell.

    python tools/sort_bench.py --tag <tag>

Shapes: one segment of n = 2^10, 2^14 and 2^18, and 4096 segments of 64.  Per shape a plan of three records -- INPUT (the keys into column
0), SORT (column 1), ARGSORT (column 2) -- and a plan of the INPUT record alone run --repeat times each; the time of a run is the one
between the HIP events the witness run records (column fills, input upload, the launches, the output gather):

    device_ms        the three-record plan: minimum and median
    input_only_ms    the INPUT record alone, same columns: minimum and median
    sort_pair_ms     the difference of the minima: the two sort records
    lexsort_ms       np.lexsort((position, value, segment)) on the host: minimum and median
    launches         of the three-record plan (fills and the output gather included)

Every shape runs in a child process of its own under `timeout -k 10`; the driver stops at the first child that does not end clean.  Each
child merges its entry into profiles/<tag>_sort.json."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
SHAPES = [(1 << 10, 1), (1 << 14, 1), (1 << 18, 1), (64, 4096)]
LIMIT_S = 180


def plans(n, segs):
    from ezkl_amd import witness_plan as WP
    total = n * segs
    k = max(4, (total - 1).bit_length())
    cells = np.arange(total, dtype=np.uint32)
    pool = np.concatenate([cells, cells, cells + (1 << k), cells + (2 << k)])       # INPUT dst, input indices = sources, SORT dst, ARGSORT dst
    recs = [[WP.INPUT, total, 0, 0, 0, total, 0, 0], [WP.SORT, total, n, 0, 2 * total, 0, 0, 0], [WP.ARGSORT, total, n, 0, 3 * total, 0, 0, 0]]
    full = WP.WitnessPlan(k, 3, total, [], [], recs, [(1 << k), (2 << k)], pool, 3 * total, 3, b"\0" * 32)
    alone = WP.WitnessPlan(k, 3, total, [], [], recs[:1], [0], pool[:2 * total], total, 1, b"\0" * 32)
    return full.validate(), alone.validate()


def child(a):
    import ezkl_amd
    from ezkl_amd import backend as B, ezkl_layout as EL
    ezkl_amd.init(0)
    n, segs = a.shape
    total = n * segs
    rng = np.random.default_rng(a.seed)
    x = rng.integers(-(1 << 20), 1 << 20, total)                                    # ties among 2^18 keys
    full, alone = plans(n, segs)
    entry = dict(n=n, segments=segs, cells=total, k=full.k)
    host = []
    seg_id, pos = np.repeat(np.arange(segs), n), np.tile(np.arange(n), segs)
    for _ in range(a.repeat):
        t = time.perf_counter()
        order = np.lexsort((pos, x, seg_id))
        host.append(1e3 * (time.perf_counter() - t))
    dev, dev0 = B.WitnessPlan(full.to_bytes()), B.WitnessPlan(alone.to_bytes())
    cols = dev.alloc_columns()
    try:
        ms, ms0 = [], []
        for i in range(a.repeat + 1):
            dev.run(x.tolist(), columns=cols)
            if i:                                                                   # the first run after the upload apart
                ms.append(dev.last["device_ms"])
            dev0.run(x.tolist(), columns=cols)
            if i:
                ms0.append(dev0.last["device_ms"])
        assert dev.last["failed"] == 0 and dev.last["cells_written"] == 3 * total
        dev.run(x.tolist(), columns=cols)                                           # (the INPUT-only plan zero-filled the columns it does not write)
        srt = cols[1].to_numpy(shape=(1 << full.k, 4))[:total]
        assert srt.tobytes() == EL.cols_to_mont([[int(v) % EL.R for v in x[order]]])[0][:total].tobytes(), "the device's sorted column is not the host's"
        entry.update(launches=dev.last["launches"], device_ms=dict(min=min(ms), median=float(np.median(ms))),
                     input_only_ms=dict(min=min(ms0), median=float(np.median(ms0))), sort_pair_ms=min(ms) - min(ms0),
                     lexsort_ms=dict(min=min(host), median=float(np.median(host))))
    finally:
        for c in cols:
            c.free()
        dev.free(); dev0.free()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    dst = os.path.join(ROOT, "profiles", "%s_sort.json" % a.tag)
    doc = json.load(open(dst)) if os.path.exists(dst) else {}
    doc["n%d_x%d" % (n, segs)] = entry
    json.dump(doc, open(dst, "w"), indent=1, sort_keys=True)
    print(json.dumps(entry))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", required=True)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--shape", type=lambda s: tuple(int(v) for v in s.split("x")), default=None, help="n x segments: one shape, in this process")
    a = ap.parse_args()
    if a.shape is not None:
        return child(a)
    for n, segs in SHAPES:                                                          # one child per shape, each under its own time limit
        cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--tag", a.tag, "--repeat", str(a.repeat), "--seed", str(a.seed),
               "--shape", "%dx%d" % (n, segs)]
        rc = subprocess.call(cmd)
        if rc != 0:
            sys.exit("sort_bench: n = %d x %d ended with status %d: nothing more is started" % (n, segs, rc))


if __name__ == "__main__":
    main()
