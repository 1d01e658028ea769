"""What checking an SRS file costs.

    python tools/srs_check_bench.py --k 16 --k 20 --tag TAG [--session 17 [--parent DIR]] [--timeout SECONDS]

per --k (one process, a test SRS made on the device by backend.gen_srs):
  * the point-check kernel alone (ezkl_hip_bases_check; HIP events around the kernel, region "bases_check"): per set, the median, minimum
    and maximum of 10 runs after a first one, and the bytes it reads (64 per point) over that time against 8 TB/s, the HBM figure this
    project uses;
  * a full check_srs of the same file, stage by stage in wall seconds with the device drained after each: upload of both sets, the two
    point checks, the window tables of both sets, the scalars, the two MSMs of the powers check, the pairing on the host, and of the
    Lagrange check its MSM on g_lagrange, the inverse NTT and the MSM on g -- next to the wall time of backend.check_srs itself, which
    builds the tables inside its first MSM on each set.
--session K: what the loaders' default adds to opening a proving session.  The artefacts of a 2^K-row MLP circuit are made once
  (tools/prove_files_bench.py's), then execute.Prover is opened in a fresh process per run, three runs per leg in the order parent (with
  --parent DIR, a built checkout of the parent commit, which knows no policy), EZKL_SRS_CHECK=off, =points; every run reports .opened,
  whose "srs_to_device" stage holds the upload, the check and the start of the table build.
Every child runs under `timeout -k 10`; one that fails ends the run.  Result: profiles/<tag>_srs_check.json."""
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
HBM_BYTES_PER_S = 8e12
SECRET = 0x5eed


def _spread(xs, digits=6):
    return dict(median=round(statistics.median(xs), digits), min=round(min(xs), digits), max=round(max(xs), digits), n=len(xs))


def size(k):
    import ezkl_amd
    from ezkl_amd import backend as B, native as NV
    ezkl_amd.init(0)
    n = 1 << k
    out = dict(k=k, points=n, kernel={})
    g, gl = B.gen_srs(k, SECRET)
    try:
        for name, b in (("g", g), ("g_lagrange", gl)):
            first = b.check()
            assert first == dict(bad=0, first_bad=None, reason=0, identities=0), first
            ms = []
            for _ in range(10):
                b.check()
                ms.append(B.last_kernel_ms("bases_check"))
            med = statistics.median(ms)
            out["kernel"][name] = dict(ms=_spread(ms), bytes_read=64 * n, tb_per_s_at_median=round(64 * n / (med * 1e-3) / 1e12, 4),
                                       share_of_8_tb_per_s=round(64 * n / (med * 1e-3) / HBM_BYTES_PER_S, 4))
        srs = dict(k=k, g=g.download(), g_lagrange=gl.download(), g2=NV.g2_mul_generator(1), s_g2=NV.g2_mul_generator(SECRET))
    finally:
        g.free(); gl.free()
    B.pool_trim()
    stages, t = {}, time.perf_counter()
    def stage(name):
        nonlocal t
        B.synchronize()
        now = time.perf_counter()
        stages[name] = round(now - t, 6)
        t = now
    key = B.srs_check_key(1)
    bg, bgl = B.Bases(srs["g"]), B.Bases(srs["g_lagrange"])
    r = v = None
    try:
        stage("upload")
        assert not bg.check()["bad"] and not bgl.check()["bad"]
        stage("point_checks")
        bg.prepare(); bgl.prepare()
        stage("window_tables")
        r, v = B.DeviceBuffer(32 * (n - 1)), B.DeviceBuffer(32 * n)
        B.chacha20_fr(key, 0, r.ptr, n - 1)
        B.chacha20_fr(key, 1, v.ptr, n)
        stage("scalars")
        a, b = B.msm_g1_dev(bg, r.ptr, n - 1, 0), B.msm_g1_dev(bg, r.ptr, n - 1, 1)
        stage("powers_msms")
        assert NV.srs_pairing_check(a, b, srs["g2"], srs["s_g2"])
        stage("pairing_host")
        left = B.msm_g1_dev(bgl, v.ptr, n)
        stage("lagrange_msm")
        w = pow(B.EvaluationDomain.ROOT, 1 << (28 - k), B._R)
        B.ntt_dev(v.ptr, k, B._to_mont(pow(w, -1, B._R)), inverse=True)
        stage("inverse_ntt")
        assert (left == B.msm_g1_dev(bg, v.ptr, n)).all()
        stage("coefficient_msm")
    finally:
        for h in (r, v, bg, bgl):
            if h is not None:
                h.free()
    out["check_srs_stages_s"] = stages
    walls = []
    for i in range(3):
        t0 = time.perf_counter()
        rep = B.check_srs(srs, seed=2 + i)
        walls.append(time.perf_counter() - t0)
        assert rep["ok"], rep
    out["check_srs_wall_s"] = dict(first=round(walls[0], 5), rest=[round(x, 5) for x in walls[1:]])
    print(json.dumps(out))


def open_once(d):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import prove_files_bench as PF
    from ezkl_amd import execute as X
    fs = PF._files(d)
    t0 = time.perf_counter()
    with X.Prover(fs["compiled"], fs["pk"], fs["srs"]) as p:
        wall = time.perf_counter() - t0
        opened = dict(p.opened)
    print(json.dumps(dict(policy=os.environ.get("EZKL_SRS_CHECK"), open_s=round(wall, 5), opened={a: round(b, 5) for a, b in opened.items()})))


def _child(args, seconds, env):
    cmd = ["timeout", "-k", "10", str(int(seconds)), sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise SystemExit("%s ended with status %d: nothing more is started" % (" ".join(cmd), r.returncode))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, action="append", default=[])
    ap.add_argument("--session", type=int, help="also: the SRS stage of execute.Prover at this k, EZKL_SRS_CHECK=points against off")
    ap.add_argument("--parent", help="(with --session) a built checkout of the parent commit, opened on the same files")
    ap.add_argument("--tag")
    ap.add_argument("--timeout", type=int, default=420, help="seconds for each child process")
    ap.add_argument("--child", choices=["size", "make", "open"])
    ap.add_argument("--dir")
    ap.add_argument("--root", help="(with --child open) the checkout whose ezkl_amd package is imported, instead of this file's own")
    a = ap.parse_args()
    if a.child:
        if a.root:
            sys.path.insert(0, os.path.abspath(a.root))
            import ezkl_amd
            if not os.path.abspath(ezkl_amd.__file__).startswith(os.path.abspath(a.root) + os.sep):
                raise SystemExit("--root: ezkl_amd was imported from %s" % ezkl_amd.__file__)
        if a.child == "size":
            size(a.k[0])
        elif a.child == "make":
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import prove_files_bench as PF
            PF.make(a.k[0], a.dir, 1)
        else:
            open_once(a.dir)
        return
    if not a.tag or not (a.k or a.session):
        ap.error("--tag and --k (or --session) are needed")
    env = dict(os.environ, ENABLE_HIP_GPU="1")
    env.pop("EZKL_SRS_CHECK", None)
    out = dict(tag=a.tag, hbm_bytes_per_s=HBM_BYTES_PER_S, sizes=[])
    path = os.path.join(ROOT, "profiles", a.tag + "_srs_check.json")
    for k in a.k:
        out["sizes"].append(_child(["--child", "size", "--k", str(k)], a.timeout, env))
        json.dump(out, open(path, "w"), indent=1)
        print("k = %d written to %s" % (k, path), flush=True)
    if a.session:
        d = tempfile.mkdtemp(prefix="srs_check_session_")
        try:
            made = _child(["--child", "make", "--k", str(a.session), "--dir", d], a.timeout, env)
            legs = ([("parent", None)] if a.parent else []) + [("off", "off"), ("points", "points")]
            runs = {name: [] for name, _ in legs}
            for _ in range(3):
                for name, policy in legs:
                    e = dict(env) if policy is None else dict(env, EZKL_SRS_CHECK=policy)
                    extra = ["--root", a.parent] if name == "parent" else []
                    runs[name].append(_child(["--child", "open", "--dir", d] + extra, a.timeout, e))
            stage = {name: [r["opened"]["srs_to_device"] for r in rs] for name, rs in runs.items()}
            out["session"] = dict(k=a.session, artefacts=made, runs=runs, srs_to_device_s={name: _spread(xs, 5) for name, xs in stage.items()},
                                  points_minus_off_median_s=round(statistics.median(stage["points"]) - statistics.median(stage["off"]), 5))
            if a.parent:
                out["session"]["off_minus_parent_median_s"] = round(statistics.median(stage["off"]) - statistics.median(stage["parent"]), 5)
            json.dump(out, open(path, "w"), indent=1)
            print("session k = %d written to %s" % (a.session, path), flush=True)
        finally:
            shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
