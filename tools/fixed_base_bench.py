"""What the fixed-base comb (csrc/g1_fixed.hip) gains over the double-and-add kernel of the parent commit.

    python tools/fixed_base_bench.py --k 12 --k 16 --k 20 --tag TAG --parent DIR [--rounds 3] [--timeout SECONDS]

DIR is a built checkout of the parent commit (its ezkl_amd package with libezkl_hip.so in it).  Per --k, n = 2^k uniform scalars on the
generator, in child processes that take turns -- parent, this tree, parent, ... -- so that both see the same sitting of the device:
  * parent: the region "bases_from_scalars" of Bases.from_scalars (the double-and-add kernel), and backend.gen_srs(k) end to end, wall ms;
  * this tree: the region "fixed_base" of backend.g1_fixed_base (the comb at EVERY n, whatever the crossover) with its part
    "fixed_base_table" (the comb kernel is the difference), "bases_from_scalars" (whichever kernel G1_FIXED_CROSSOVER picks), gen_srs.
Every figure is the median, minimum and maximum over the rounds' runs (5 per child after one that is not counted).  Every child runs under
`timeout -k 10`; one that fails ends the run.  (--k 0 times one product; its gen_srs figure is that of k = 1, the smallest SRS.)
Result: profiles/<tag>_fixed_base.json, with the window width and the crossover of this tree, who shares an inversion, and the device's
field-product rate (ezkl_hip_ubench "modmul")."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
SECRET = 0x5eed
RUNS = 5


def size(root, ks):
    sys.path.insert(0, root)
    import numpy as np
    import ezkl_amd
    from ezkl_amd import backend as B
    ezkl_amd.init(0)
    comb = hasattr(B, "g1_fixed_base")
    G = np.frombuffer((B._MONT % B._Q).to_bytes(32, "little") + (2 * B._MONT % B._Q).to_bytes(32, "little"), np.uint64).copy()
    out = dict(comb=comb, sizes={})
    if comb:
        out.update(c=B.G1_FIXED_C, crossover=B.G1_FIXED_CROSSOVER, modmul_per_s=B.ubench("modmul"))
    for k in ks:
        n = 1 << k
        sc, pts = B.DeviceBuffer(32 * n), B.DeviceBuffer(64 * n)
        B.chacha20_fr(bytes(range(32)), 0, sc.ptr, n)
        ms = {"bases_from_scalars": [], "fixed_base": [], "fixed_base_table": [], "gen_srs_wall": []}
        for i in range(RUNS + 1):                                        # the first turn of each is not counted
            B.Bases.from_scalars(G, sc.ptr, n).free()
            got = {"bases_from_scalars": B.last_kernel_ms("bases_from_scalars")}
            if comb:
                B.g1_fixed_base(G, sc.ptr, n, pts.ptr)
                got.update({r: B.last_kernel_ms(r) for r in ("fixed_base", "fixed_base_table")})
            B.synchronize()
            t0 = time.perf_counter()
            g, gl = B.gen_srs(max(k, 1), SECRET)
            B.synchronize()
            got["gen_srs_wall"] = (time.perf_counter() - t0) * 1e3
            g.free(); gl.free()
            if i:
                for r, v in got.items():
                    ms[r].append(v)
        sc.free(); pts.free()
        out["sizes"][str(k)] = {r: xs for r, xs in ms.items() if xs}
    print(json.dumps(out))


def _child(root, ks, seconds):
    cmd = ["timeout", "-k", "10", str(int(seconds)), sys.executable, os.path.abspath(__file__), "--child", "--root", root]
    for k in ks:
        cmd += ["--k", str(k)]
    env = dict(os.environ, ENABLE_HIP_GPU="1")
    env.pop("EZKL_HIP_LIB", None)
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise SystemExit("%s ended with status %d: nothing more is started" % (" ".join(cmd), r.returncode))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def _spread(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4), n=len(xs))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, action="append", default=[])
    ap.add_argument("--tag")
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300, help="seconds for each child process")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        size(a.root, a.k)
        return
    if not a.tag or not a.k or not a.parent:
        ap.error("--tag, --parent and --k are needed")
    legs = {"parent": os.path.abspath(a.parent), "here": ROOT}
    raw = {leg: {str(k): {} for k in a.k} for leg in legs}
    facts = {}
    for _ in range(a.rounds):
        for leg, root in legs.items():
            got = _child(root, a.k, a.timeout)
            if leg == "here":
                facts = {f: got[f] for f in ("c", "crossover", "modmul_per_s")}
            for k, regions in got["sizes"].items():
                for r, xs in regions.items():
                    raw[leg][k].setdefault(r, []).extend(xs)
    out = dict(tag=a.tag, window_bits=facts["c"], crossover=facts["crossover"], inversion_shared_by="workgroup (4 waves; per wave measured slower, DESIGN.md)",
               field_products_per_s=facts["modmul_per_s"], sizes=[])
    for k in a.k:
        p, h = raw["parent"][str(k)], raw["here"][str(k)]
        row = dict(k=k, n=1 << k, parent={r: _spread(xs) for r, xs in p.items()}, here={r: _spread(xs) for r, xs in h.items()})
        comb = [t - tb for t, tb in zip(h["fixed_base"], h["fixed_base_table"])]
        row["here"]["fixed_base_comb"] = _spread(comb)
        row["speedup_fixed_base"] = round(statistics.median(p["bases_from_scalars"]) / statistics.median(h["fixed_base"]), 3)
        row["speedup_gen_srs"] = round(statistics.median(p["gen_srs_wall"]) / statistics.median(h["gen_srs_wall"]), 3)
        out["sizes"].append(row)
    path = os.path.join(ROOT, "profiles", a.tag + "_fixed_base.json")
    json.dump(out, open(path, "w"), indent=1)
    print(json.dumps(out))
    print("written to %s" % path)


if __name__ == "__main__":
    main()
