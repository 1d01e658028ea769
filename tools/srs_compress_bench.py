"""What decompressing the points of a processed SRS file costs.

    python tools/srs_compress_bench.py --k 16 --k 20 --tag TAG [--timeout SECONDS]

per --k (one process, a test SRS made on the device by backend.gen_srs, compressed by Bases.compressed):
  * the decompression kernel alone (HIP events around it, region "g1_decompress") for every window-table form of csrc/g1_compress.hip
    (ezkl_hip_g1_decompress_form_dev), turn about: the median, minimum and maximum of 10 runs after a first one; the products per second
    that makes (251 squarings + 54 products per point with a table, + 108 without, and the 9 around the chain) against the product roof
    ezkl_hip_ubench measures in the same process ("modmul29", and "modmul29_o4" at four waves per SIMD); the compression kernel likewise;
  * execute.decompress_srs of the processed file by stage -- read and parse, both sets through Bases.from_compressed, the download,
    writing the raw file -- wall seconds, the device drained after each;
  * opening a Prover session of the golden k = 6 MLP (the file is downsized to it, the normal case of a shared SRS file) on the processed
    file and on the raw file of the same SRS, turn about, three each.
Every child runs under `timeout -k 10`; one that fails ends the run.  Result: profiles/<tag>_srs_compress.json."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
SECRET = 0x5eed
FORMS = {0: "registers, unrolled", 1: "LDS, unrolled", 2: "no table (binary chain), unrolled", 3: "registers, squaring runs as loops", 4: "LDS, squaring runs as loops"}


def _spread(xs, digits=4):
    return dict(median=round(statistics.median(xs), digits), min=round(min(xs), digits), max=round(max(xs), digits), n=len(xs))


def size(k):
    import numpy as np
    import ezkl_amd
    import gen_fq_sqrt_chain as GEN
    from ezkl_amd import backend as B, codecs, execute as X, lib as L, native as NV
    ezkl_amd.init(0)
    n = 1 << k
    out = dict(k=k, points=n)
    g, gl = B.gen_srs(k, SECRET)
    raw = dict(k=k, g=g.download(), g_lagrange=gl.download(), g2=NV.g2_mul_generator(1), s_g2=NV.g2_mul_generator(SECRET))
    ms = []
    for i in range(11):
        data = g.compressed()
        if i:
            ms.append(B.last_kernel_ms("g1_compress"))
    out["compress_kernel_ms"] = _spread(ms)
    packed = dict(raw, g=np.frombuffer(data, np.uint8).reshape(n, 32), g_lagrange=np.frombuffer(gl.compressed(), np.uint8).reshape(n, 32))
    g.free(); gl.free()
    src, dst = B.DeviceBuffer.from_numpy(packed["g"]), B.DeviceBuffer(64 * n)
    bad, why = C.c_uint64(0), C.c_int(0)
    ms = {f: [] for f in FORMS}
    for i in range(11):                                                 # the first turn of each is not counted
        for f in FORMS:
            L.check(L.load().ezkl_hip_g1_decompress_form_dev(C.c_void_p(src.ptr), C.c_size_t(n), C.c_int(f), C.c_void_p(dst.ptr), C.byref(bad), C.byref(why)), "form")
            assert why.value == 0
            if i == 0:
                assert dst.to_numpy(shape=(n, 8)).tobytes() == raw["g"].tobytes(), "form %d" % f
            else:
                ms[f].append(B.last_kernel_ms("g1_decompress"))
    src.free(); dst.free()
    roof = {w: B.ubench(w) for w in ("modmul29", "modmul29_o4", "modmul29_o2")}
    out["product_roof_per_s"] = {w: float("%.4g" % v) for w, v in roof.items()}
    out["decompress_kernel"] = {}
    for f, xs in ms.items():
        w = 1 if f == 2 else GEN.WINDOW
        sq, mul = GEN.counts(GEN.chain(GEN.E, w), w)
        products = sq + mul + 9                                          # around the chain: to Montgomery form, x^3 (2), y^2, the parity's and two conversions out
        rate = products * n / (statistics.median(xs) * 1e-3)
        out["decompress_kernel"][str(f)] = dict(form=FORMS[f], ms=_spread(xs), products_per_point=products, products_per_s=float("%.4g" % rate),
                                                fraction_of_roof=round(rate / roof["modmul29"], 3))
    B.pool_trim()
    with tempfile.TemporaryDirectory() as d:
        p_raw, p_packed, p_back = (os.path.join(d, x) for x in ("raw.srs", "processed.srs", "back.srs"))
        open(p_raw, "wb").write(codecs.write_srs(raw))
        open(p_packed, "wb").write(codecs.write_srs(packed))
        stages, t = {}, time.perf_counter()

        def lap(name):
            nonlocal t
            B.synchronize()
            now = time.perf_counter()
            stages[name] = round(now - t, 5)
            t = now
        srs = codecs.read_srs(open(p_packed, "rb").read()); lap("read_and_parse")
        sets = [B.Bases.from_compressed(srs[name], name) for name in ("g", "g_lagrange")]; lap("decompress_both_sets")
        arrays = [b.download() for b in sets]; lap("download")
        open(p_back, "wb").write(codecs.write_srs(dict(srs, g=arrays[0], g_lagrange=arrays[1]))); lap("write")
        for b in sets:
            b.free()
        assert open(p_back, "rb").read() == open(p_raw, "rb").read()
        out["decompress_srs_stages_s"] = stages
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            X.decompress_srs(p_packed, p_back)
            walls.append(round(time.perf_counter() - t0, 5))
        out["decompress_srs_wall_s"] = walls
        compiled, pk = os.path.join(ROOT, "tests", "golden", "model_k6.compiled"), os.path.join(d, "pk.key")
        X.setup(compiled, p_raw, os.path.join(d, "vk.key"), pk)
        opens = {"raw": [], "processed": []}
        for _ in range(3):
            for name, path in (("raw", p_raw), ("processed", p_packed)):
                t0 = time.perf_counter()
                with X.Prover(compiled, pk, path):
                    B.synchronize()
                opens[name].append(round(time.perf_counter() - t0, 5))
        out["prover_open_s"] = opens
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
    path = os.path.join(ROOT, "profiles", a.tag + "_srs_compress.json")
    for k in a.k:
        out["sizes"].append(_child(["--child", "size", "--k", str(k)], a.timeout, env))
        json.dump(out, open(path, "w"), indent=1)
        print("k = %d written to %s" % (k, path), flush=True)


if __name__ == "__main__":
    main()
