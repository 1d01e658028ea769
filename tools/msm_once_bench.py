"""What an MSM without window tables costs, and what it saves a caller that uses a base set once.

    python tools/msm_once_bench.py --k 16 --k 20 --tag TAG [--parent DIR] [--timeout SECONDS]

per --k, every leg in a process of its own (`timeout -k 10`; one that fails ends the run), 10 runs after a first one, median and range:
  (a) first    a FRESH handle (the same 2^k generated points every run) to its first MSM result, uniform scalars.  This tree:
               Bases.msm_once.  --parent DIR (a built checkout of the parent commit): Bases.prepare and the first fixed-base MSM.  Wall
               milliseconds around the calls with the device drained before them -- the table build runs on a stream of the library's own,
               which no event pair of the caller's brackets; the call returns with the point, so the host tail is inside for both -- and,
               for this tree, the HIP events around the device work as well (region "msm_once").
  (b) check    backend.check_srs as one call on a test SRS of 2^k points made on the device (backend.gen_srs), wall seconds, this tree
               and the parent.
  (c) steady   for the record (the reason the path is not the default): on ONE prepared handle, a fixed-base MSM (HIP events, region
               "msm") against a table-free MSM (region "msm_once"), on uniform and on witness-like scalars (70 % +-20-bit, 20 % zero).
Verdicts in the result: a_once_below_parent[k] (the whole table-free range lies below the parent's), b_not_slower[k] (this tree's median
is not above the parent's maximum).  Result: profiles/<tag>_msm_once.json."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
SEED = 0x657a6b6c
SECRET = 0x5eed
RUNS = 10
R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001


def _spread(xs, digits=4):
    return dict(median=round(statistics.median(xs), digits), min=round(min(xs), digits), max=round(max(xs), digits), n=len(xs))


def _uniform(rng, n):
    import numpy as np
    a = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 61) - 1)               # 253 random bits: below r
    return a


def _witness_like(B, rng, n):
    """Montgomery words of 70 % uniform values in (-2^20, 2^20), 20 % zeros, 10 % uniform field elements: made on the device from integers"""
    import numpy as np
    v = rng.integers(-(1 << 20) + 1, 1 << 20, size=n).astype(np.int64)
    kind = rng.random(n)
    v[kind >= 0.7] = 0
    neg = v < 0
    words = np.zeros((n, 4), np.uint64)
    words[:, 0] = np.abs(v).astype(np.uint64)
    rl = np.frombuffer(R.to_bytes(32, "little"), np.uint64)
    # r - |x| for the negatives: |x| < 2^20 <= r's low limb, so only that limb changes
    words[neg] = rl
    words[neg, 0] = rl[0] - np.abs(v[neg]).astype(np.uint64)
    u = _uniform(rng, n)
    d = B.DeviceBuffer.from_numpy(words)
    B.vec_scale(d.ptr, B._to_mont((1 << 256) % R), d.ptr, n)       # canonical words -> Montgomery words: a Montgomery product with the words of 2^512 mod r
    out = d.to_numpy(shape=(n, 4))
    d.free()
    for i in (0, 1, n // 2, n - 1):
        assert out[i].tobytes() == B._to_mont(int(v[i]) % R).tobytes(), i
    out[kind >= 0.9] = u[kind >= 0.9]
    return out


def first(k, parent):
    import numpy as np
    import ezkl_amd
    from ezkl_amd import backend as B
    ezkl_amd.init(0)
    n = 1 << k
    d = B.DeviceBuffer.from_numpy(_uniform(np.random.default_rng(k), n))
    wall, events, point = [], [], None
    for i in range(RUNS + 1):
        b = B.Bases.generate(SEED, n)
        B.synchronize()
        t0 = time.perf_counter()
        if parent:
            b.prepare()
            p = B.msm_g1_dev(b, d.ptr, n)
        else:
            p = b.msm_once(d.ptr)
        t = (time.perf_counter() - t0) * 1e3
        if not parent:
            assert not b.has_table()
            events.append(B.last_kernel_ms("msm_once"))
        b.free()
        assert point is None or (p == point).all()
        point = p
        if i:
            wall.append(t)
    out = dict(k=k, leg="parent: prepare + first fixed-base MSM" if parent else "table-free MSM", wall_ms=_spread(wall), point=point.tobytes().hex())
    if events:
        out["event_ms"] = _spread(events[1:])
    d.free()
    print(json.dumps(out))


def check(k):
    import ezkl_amd
    from ezkl_amd import backend as B, native as NV
    ezkl_amd.init(0)
    g, gl = B.gen_srs(k, SECRET)
    try:
        srs = dict(k=k, g=g.download(), g_lagrange=gl.download(), g2=NV.g2_mul_generator(1), s_g2=NV.g2_mul_generator(SECRET))
    finally:
        g.free(); gl.free()
    B.pool_trim()
    walls = []
    for i in range(RUNS + 1):
        B.synchronize()
        t0 = time.perf_counter()
        rep = B.check_srs(srs, seed=2 + i)
        t = time.perf_counter() - t0
        assert rep["ok"], rep
        if i:
            walls.append(t)
    print(json.dumps(dict(k=k, check_srs_wall_s=_spread(walls, 5))))


def steady(k):
    import numpy as np
    import ezkl_amd
    from ezkl_amd import backend as B
    ezkl_amd.init(0)
    n = 1 << k
    b = B.Bases.generate(SEED, n)
    out = dict(k=k)
    try:
        b.prepare()
        rng = np.random.default_rng(100 + k)
        for name, s in (("uniform", _uniform(rng, n)), ("witness_like", _witness_like(B, rng, n))):
            d = B.DeviceBuffer.from_numpy(s)
            fixed, once = [], []
            for i in range(RUNS + 1):
                p = b.msm(d.ptr)
                fixed.append(B.last_kernel_ms("msm"))
                q = b.msm_once(d.ptr)
                once.append(B.last_kernel_ms("msm_once"))
                assert (p == q).all()
            d.free()
            out[name] = dict(fixed_base_event_ms=_spread(fixed[1:]), table_free_event_ms=_spread(once[1:]),
                             ratio_of_medians=round(statistics.median(once[1:]) / statistics.median(fixed[1:]), 2))
    finally:
        b.free()
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
    ap.add_argument("--parent", help="a built checkout of the parent commit: its prepare + first MSM in (a), its check_srs in (b)")
    ap.add_argument("--tag")
    ap.add_argument("--timeout", type=int, default=240, help="seconds for each child process")
    ap.add_argument("--child", choices=["first", "check", "steady"])
    ap.add_argument("--root", help="(with --child) the checkout whose ezkl_amd package is imported, instead of this file's own")
    a = ap.parse_args()
    if a.child:
        root = os.path.abspath(a.root) if a.root else ROOT
        sys.path.insert(0, root)
        import ezkl_amd
        if not os.path.abspath(ezkl_amd.__file__).startswith(root + os.sep):
            raise SystemExit("ezkl_amd was imported from %s, not from %s" % (ezkl_amd.__file__, root))
        if a.child == "first":
            first(a.k[0], parent=bool(a.root))
        elif a.child == "check":
            check(a.k[0])
        else:
            steady(a.k[0])
        return
    if not a.tag or not a.k:
        ap.error("--tag and --k are needed")
    env = dict(os.environ, ENABLE_HIP_GPU="1")
    out = dict(tag=a.tag, runs=RUNS, sizes=[], a_once_below_parent={}, b_not_slower={})
    path = os.path.join(ROOT, "profiles", a.tag + "_msm_once.json")
    parent = ["--root", os.path.abspath(a.parent)] if a.parent else None
    for k in a.k:
        ks = ["--k", str(k)]
        size = dict(k=k, points=1 << k)
        size["first"] = dict(this=_child(["--child", "first"] + ks, a.timeout, env))
        size["check_srs"] = dict(this=_child(["--child", "check"] + ks, a.timeout, env))
        if parent:
            size["first"]["parent"] = _child(["--child", "first"] + ks + parent, a.timeout, env)
            size["check_srs"]["parent"] = _child(["--child", "check"] + ks + parent, a.timeout, env)
            assert size["first"]["this"].pop("point") == size["first"]["parent"].pop("point"), "the two trees computed different points"
            out["a_once_below_parent"][str(k)] = size["first"]["this"]["wall_ms"]["max"] < size["first"]["parent"]["wall_ms"]["min"]
            out["b_not_slower"][str(k)] = size["check_srs"]["this"]["check_srs_wall_s"]["median"] <= size["check_srs"]["parent"]["check_srs_wall_s"]["max"]
        size["steady"] = _child(["--child", "steady"] + ks, a.timeout, env)
        out["sizes"].append(size)
        json.dump(out, open(path, "w"), indent=1)
        print("k = %d written to %s" % (k, path), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
