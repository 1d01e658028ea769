#!/usr/bin/env python3
"""The G2 MSM's two kernels against each other, and the crossover of ezkl_hip_msm_g2.

    python tools/msm_g2_bench.py --tag TAG [--parent DIR] [--k 4 --k 5 ...] [--timeout SECONDS]

For every n = 2^k (default k = 4 .. 16), one child process per leg, each under its own `timeout -k 10`; a leg that fails ends the run:
  chain    this tree, backend.msm_g2_points on resident points and scalars: the bucket chain.  Wall time of the call (it returns after the
           stream has drained) and the HIP events around the device work (region "msm_g2").
  naive    --parent DIR (a built checkout of the parent commit): its backend.msm_g2, the double-and-add kernel at every n.  Wall time of the
           call, which includes its four allocations and the upload of n x 160 bytes.
  host     this tree, backend.msm_g2 (host pointers): upload + whichever kernel MSM_G2_CROSSOVER picks.
RUNS timed calls after one that is not timed; median, minimum and maximum.  The three legs must return the same 128 bytes.
`crossover`: the smallest 2^k from which the chain's MAXIMUM is below the naive leg's MINIMUM at that size and every larger one.
Result: profiles/<tag>_msm_g2.json."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
RUNS = 7


def _spread(xs, digits=4):
    return dict(median=round(statistics.median(xs), digits), min=round(min(xs), digits), max=round(max(xs), digits), n=len(xs))


def _inputs(k):
    """n points picked from eight multiples of the generator (one of them the identity record), n uniform 253-bit scalars as Montgomery words"""
    import numpy as np
    from ezkl_amd import native as NV
    n, rng = 1 << k, np.random.default_rng(k)
    base = np.stack([np.frombuffer(NV.g2_mul_generator(m), np.uint64) if m else np.zeros(16, np.uint64) for m in (1, 2, 3, 5, 7, 11, 13, 0)])
    s = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    s[:, 3] &= np.uint64((1 << 61) - 1)
    return np.ascontiguousarray(base[rng.integers(0, 8, n)]), s


def leg(k, which):
    import ezkl_amd
    from ezkl_amd import backend as B
    ezkl_amd.init(0)
    pts, s = _inputs(k)
    wall, events, point = [], [], None
    if which == "chain":
        dp, ds = B.DeviceBuffer.from_numpy(pts), B.DeviceBuffer.from_numpy(s)
    for i in range(RUNS + 1):
        B.synchronize()
        t0 = time.perf_counter()
        p = B.msm_g2_points(dp, ds) if which == "chain" else B.msm_g2(pts, s)
        t = (time.perf_counter() - t0) * 1e3
        if which == "chain":
            events.append(B.last_kernel_ms("msm_g2"))
        assert point is None or (p == point).all()
        point = p
        if i:
            wall.append(t)
    out = dict(k=k, leg=which, wall_ms=_spread(wall), point=point.tobytes().hex())
    if events:
        out["event_ms"] = _spread(events[1:])
    print(json.dumps(out))


def _child(args, seconds, env):
    cmd = ["timeout", "-k", "10", str(int(seconds)), sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise SystemExit("%s ended with status %d: nothing more is started" % (" ".join(cmd), r.returncode))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, action="append", default=[])
    ap.add_argument("--parent", help="a built checkout of the parent commit: the double-and-add kernel at every size")
    ap.add_argument("--tag")
    ap.add_argument("--timeout", type=int, default=120, help="seconds for each child process")
    ap.add_argument("--child", choices=["chain", "naive", "host"])
    ap.add_argument("--root", help="(with --child) the checkout whose ezkl_amd package is imported, instead of this file's own")
    a = ap.parse_args()
    if a.child:
        root = os.path.abspath(a.root) if a.root else ROOT
        sys.path.insert(0, root)
        import ezkl_amd
        if not os.path.abspath(ezkl_amd.__file__).startswith(root + os.sep):
            raise SystemExit("ezkl_amd was imported from %s, not from %s" % (ezkl_amd.__file__, root))
        leg(a.k[0], a.child)
        return
    if not a.tag:
        ap.error("--tag is needed")
    env = dict(os.environ, ENABLE_HIP_GPU="1")
    rows = []
    for k in a.k or list(range(4, 17)):
        ks = ["--k", str(k)]
        row = dict(k=k, points=1 << k, chain=_child(["--child", "chain"] + ks, a.timeout, env), host=_child(["--child", "host"] + ks, a.timeout, env))
        if a.parent:
            row["naive"] = _child(["--child", "naive"] + ks + ["--root", os.path.abspath(a.parent)], a.timeout, env)
        points = {row[l].pop("point") for l in ("chain", "host", "naive") if l in row}
        assert len(points) == 1, "the legs disagree at k = %d" % k
        if a.parent:
            row["naive_over_chain"] = round(row["naive"]["wall_ms"]["median"] / row["chain"]["wall_ms"]["median"], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = dict(tag=a.tag, runs=RUNS, sizes=rows)
    if a.parent:
        wins = [r["chain"]["wall_ms"]["max"] < r["naive"]["wall_ms"]["min"] for r in rows]
        first = next((i for i in range(len(rows)) if all(wins[i:])), None)
        out["crossover"] = None if first is None else rows[first]["points"]
    path = os.path.join(ROOT, "profiles", a.tag + "_msm_g2.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path, "crossover:", out.get("crossover"))


if __name__ == "__main__":
    main()
