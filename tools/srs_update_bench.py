"""What an SRS update costs.

    python tools/srs_update_bench.py --k 16 --k 20 --tag TAG [--timeout SECONDS]

per --k (one process, a test SRS made on the device by backend.gen_srs):
  * the per-row product kernel alone (ezkl_hip_bases_mul_scalars; HIP events around the kernel, region "bases_mul_scalars") on g with
    the scalars t^i, and in the same run, turn about, the fixed-base kernel (ezkl_hip_bases_from_scalars, region "bases_from_scalars")
    on the same scalars: the median, minimum and maximum of 10 runs of each after a first one, and the ratio of the medians.  The two
    do the same count of group operations; the new one holds its point in vector registers and reads it from memory;
  * a whole backend.update_srs by stage, wall seconds with the device drained after each (upload of g, the powers of t, the per-row
    product, the inverse NTT over G1, the two G2 products, the download of both sets), next to its wall time as one call without
    those waits, three calls;
  * a whole backend.verify_srs_update of that update, wall seconds, three calls.
Every child runs under `timeout -k 10`; one that fails ends the run.  Result: profiles/<tag>_srs_update.json."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
SECRET = 0x5eed
T = 0x1f2e3d4c5b6a79880796a5b4c3d2e1f00f1e2d3c4b5a69788796a5b4c3d2e1f0          # a full-width update secret


def _spread(xs, digits=6):
    return dict(median=round(statistics.median(xs), digits), min=round(min(xs), digits), max=round(max(xs), digits), n=len(xs))


def size(k):
    import numpy as np
    import ezkl_amd
    from ezkl_amd import backend as B, native as NV
    ezkl_amd.init(0)
    n = 1 << k
    out = dict(k=k, points=n)
    g, gl = B.gen_srs(k, SECRET)
    tpow = B.DeviceBuffer(32 * n)
    try:
        B.vec_fill(tpow.ptr, B._to_mont(T), n)
        B.prefix_scan("mul", tpow.ptr, tpow.ptr, n, exclusive=True)
        G = g.download()[0].copy()                                      # g[0] = G: the fixed base of the comparison
        ms = {"bases_mul_scalars": [], "bases_from_scalars": []}
        for i in range(11):                                             # the first turn of each is not counted
            for region, run in (("bases_mul_scalars", lambda: g.mul_scalars(tpow.ptr)), ("bases_from_scalars", lambda: B.Bases.from_scalars(G, tpow.ptr, n))):
                b = run()
                if i:
                    ms[region].append(B.last_kernel_ms(region))
                b.free()
        out["kernel_ms"] = {region: _spread(xs, 4) for region, xs in ms.items()}
        out["mul_scalars_over_from_scalars"] = round(statistics.median(ms["bases_mul_scalars"]) / statistics.median(ms["bases_from_scalars"]), 4)
        srs = dict(k=k, g=g.download(), g_lagrange=gl.download(), g2=NV.g2_mul_generator(1), s_g2=NV.g2_mul_generator(SECRET))
    finally:
        tpow.free(); g.free(); gl.free()
    B.pool_trim()
    stages = {}
    t0 = time.perf_counter()
    new, proof = B.update_srs(srs, T, stages=stages)
    out["update_srs_stages_s"] = {a: round(b, 6) for a, b in stages.items()}
    out["update_srs_staged_wall_s"] = round(time.perf_counter() - t0, 5)
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        again, _p = B.update_srs(srs, T)
        walls.append(time.perf_counter() - t0)
    assert np.array_equal(again["g"], new["g"]) and np.array_equal(again["g_lagrange"], new["g_lagrange"]) and again["s_g2"] == new["s_g2"]
    out["update_srs_wall_s"] = [round(x, 5) for x in walls]
    walls = []
    for i in range(3):
        t0 = time.perf_counter()
        rep = B.verify_srs_update(srs, new, proof, seed=2 + i)
        walls.append(time.perf_counter() - t0)
        assert rep["ok"], rep
    out["verify_srs_update_wall_s"] = dict(first=round(walls[0], 5), rest=[round(x, 5) for x in walls[1:]])
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
    ap.add_argument("--tag")
    ap.add_argument("--timeout", type=int, default=300, help="seconds for each child process")
    ap.add_argument("--child", choices=["size"])
    a = ap.parse_args()
    if a.child:
        size(a.k[0])
        return
    if not a.tag or not a.k:
        ap.error("--tag and --k are needed")
    env = dict(os.environ, ENABLE_HIP_GPU="1")
    env.pop("EZKL_SRS_CHECK", None)
    out = dict(tag=a.tag, sizes=[])
    path = os.path.join(ROOT, "profiles", a.tag + "_srs_update.json")
    for k in a.k:
        out["sizes"].append(_child(["--child", "size", "--k", str(k)], a.timeout, env))
        json.dump(out, open(path, "w"), indent=1)
        print("k = %d written to %s" % (k, path), flush=True)


if __name__ == "__main__":
    main()
