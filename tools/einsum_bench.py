"""The claimed product of an einsum -- a DOT record of ONE step -- replayed by this library (wit_dot_wide_kernel from DOT_WIDE_MIN
products on) and by the parent commit's library (wit_dot_kernel, 1 lane in 16 at work) from the SAME plan blob, and the attention head's
witness replayed both ways.

    python tools/einsum_bench.py --tag <tag> --parent <built checkout of the parent commit>

Legs, each a child process of its own under `timeout -k 10`, one after the other; the driver stops at the first that does not end clean:

    dots       synthetic plans of 300 full-range constants and ONE DOT record, p1 = 1, count = 4096, p0 in 16, 24, 32, 48, 64, 128, 256, 512,
               and `floor`, the same plan without the DOT record.  The blobs are written once by the driver (profiles/<tag>_einsum_blobs/) and
               read by both libraries' children.
    attention  AttentionHeadCircuit at n = 64, e = 64, d = 32 (k = 17): both phases of its recorded plan; and its five claims record by
               record, as synthetic one-record plans of their (count, p0).

A time is that of a whole `run` between the HIP events the library records around it (ezkl_hip_last_kernel_ms("witness")): the column
fills, the records, the status read-back.  Per plan: --repeat runs after a first one, in each of --sittings uploads of the plan; `ms` is the
median of the sitting medians, `spread` the greatest distance of a sitting median from it.  A DOT record's own cost is ms - floor.  The
children of this library also read the wide-kernel counter, and every entry carries `columns`, the SHA-256 of all advice columns after the
last run: the two libraries must agree on it, and the driver fails when they do not.  Everything goes to profiles/<tag>_einsum.json."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
COUNT, WIDTHS, N_SRC, K_DOTS = 4096, (16, 24, 32, 48, 64, 128, 256, 512), 300, 13
ATT = dict(k=17, n=64, e=64, d=32, blocks=4, decomp_base=1024)
LIMIT_S = 420


def dot_blob(p0, count, seed=1, k=K_DOTS):
    """300 full-range constants in column 0, `count` one-step dots of p0 products over random cells of them into column 1 (p0 = 0: none)"""
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    rng = np.random.default_rng(seed)
    consts = [int.from_bytes(rng.bytes(32), "little") % EL.R for _ in range(N_SRC)]
    src = np.arange(N_SRC, dtype=np.uint32)
    records, pool, cells = [[WP.CONST, N_SRC, 0, 0, 0, N_SRC, 0, 0]], [src, src], N_SRC
    if p0:
        a, b = (rng.integers(0, N_SRC, p0 * count).astype(np.uint32) for _ in range(2))
        dst = (1 << k) + np.arange(count, dtype=np.uint32)
        o = 2 * N_SRC
        records.append([WP.DOT, count, p0, 1, o, o + count, o + count + p0 * count, 0])
        pool, cells = pool + [dst, a, b], cells + count
    return WP.WitnessPlan(k, 2, 0, [], consts, records, [], np.concatenate(pool), cells, len(records), b"\0" * 32).validate().to_bytes()


def attention():
    from ezkl_amd import ezkl_layout as EL
    return EL.AttentionHeadCircuit(ATT["k"], ATT["n"], ATT["e"], ATT["d"], capacity=ATT["blocks"] << ATT["k"], decomp_base=ATT["decomp_base"])


def timed(B, blob, inputs, repeat, sittings, challenges=()):
    """-> per phase dict(ms, spread, sittings), the wide launches of one run (None: a library without the counter), the digest of the columns"""
    from ezkl_amd import lib
    counted = hasattr(lib.load(), "ezkl_hip_witness_wide_dots")
    per_phase, wide, digest = {}, None, None
    for _ in range(sittings):
        dev = B.WitnessPlan(blob)
        cols = dev.alloc_columns()
        try:
            phases = [None] if dev.n_phases == 1 else list(range(dev.n_phases))
            ms = {p: [] for p in phases}
            for i in range(repeat + 1):
                if counted:
                    B.witness_wide_dots(reset=True)
                for p in phases:
                    dev.run(inputs, columns=cols, phase=p, challenges=challenges if p else ())
                    assert dev.last["failed"] == 0
                    if i:                                                           # the first run after the upload apart
                        ms[p].append(dev.last["device_ms"])
                wide = B.witness_wide_dots() if counted else None
            for p in phases:
                per_phase.setdefault(p, []).append(float(np.median(ms[p])))
            h = hashlib.sha256()
            for col in cols:
                h.update(col.to_numpy(shape=(1 << dev.k, 4)).tobytes())
            assert digest in (None, h.hexdigest()), "two sittings wrote different columns"
            digest = h.hexdigest()
        finally:
            for col in cols:
                col.free()
            dev.free()
    out = {}
    for p, meds in per_phase.items():
        mid = float(np.median(meds))
        out["run" if p is None else "phase%d" % p] = dict(ms=mid, spread=max(abs(v - mid) for v in meds), sittings=meds)
    return out, wide, digest


def child(a):
    import ezkl_amd
    from ezkl_amd import backend as B, lib
    ezkl_amd.init(0)
    blobs = os.path.join(ROOT, "profiles", "%s_einsum_blobs" % a.tag)
    entry = dict(library=os.path.relpath(lib.lib_path(), ROOT))
    if a.leg == "dots":
        for name in ["floor"] + ["p0_%d" % w for w in WIDTHS]:
            t, wide, digest = timed(B, open(os.path.join(blobs, name + ".wplan"), "rb").read(), [], a.repeat, a.sittings)
            entry[name] = dict(t["run"], wide_launches=wide, columns=digest)
    else:
        meta = json.load(open(os.path.join(blobs, "attention.json")))
        t, wide, digest = timed(B, open(os.path.join(blobs, "attention.wplan"), "rb").read(), meta["inputs"], a.repeat, a.sittings, meta["challenges"])
        entry["replay"] = dict(t, wide_launches=wide, columns=digest, records=meta["records"], cells=meta["cells"])
        for count, p0 in meta["claims"]:
            t, wide, digest = timed(B, open(os.path.join(blobs, "claim_%dx%d.wplan" % (count, p0)), "rb").read(), [], a.repeat, a.sittings)
            entry["claim_%dx%d" % (count, p0)] = dict(t["run"], wide_launches=wide, columns=digest)
        t, _, digest = timed(B, open(os.path.join(blobs, "claim_floor.wplan"), "rb").read(), [], a.repeat, a.sittings)
        entry["claim_floor"] = dict(t["run"], columns=digest)
    dst = os.path.join(ROOT, "profiles", "%s_einsum.json" % a.tag)
    doc = json.load(open(dst)) if os.path.exists(dst) else {}
    doc.setdefault(a.leg, {})[a.side] = entry
    json.dump(doc, open(dst, "w"), indent=1, sort_keys=True)
    print(json.dumps({a.leg: {a.side: entry}}))


def write_blobs(tag):
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    blobs = os.path.join(ROOT, "profiles", "%s_einsum_blobs" % tag)
    os.makedirs(blobs, exist_ok=True)
    put = lambda name, blob: open(os.path.join(blobs, name), "wb").write(blob)
    put("floor.wplan", dot_blob(0, COUNT))
    for w in WIDTHS:
        put("p0_%d.wplan" % w, dot_blob(w, COUNT))
    c = attention()
    plan = WP.record_plan(c).validate()
    put("attention.wplan", plan.to_bytes())
    claims = sorted(set((int(r[1]), int(r[2])) for r in plan.records if r[0] == WP.DOT and r[7] == 0 and r[3] == 1 and r[2] >= 16))
    for count, p0 in claims:
        put("claim_%dx%d.wplan" % (count, p0), dot_blob(p0, count, k=ATT["k"]))
    put("claim_floor.wplan", dot_blob(0, COUNT, k=ATT["k"]))
    meta = dict(inputs=c.default_inputs(), challenges=[0x1234567890abcdef1234567890abcdef % EL.R, 0xfedcba0987654321 % EL.R], claims=claims,
                records=int(plan.n_records), cells=int(plan.n_cells))
    json.dump(meta, open(os.path.join(blobs, "attention.json"), "w"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", required=True)
    ap.add_argument("--parent", help="a built checkout of the parent commit: its ezkl_amd/libezkl_hip.so replays the same blobs")
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--sittings", type=int, default=5)
    ap.add_argument("--leg", choices=["dots", "attention"], help="one leg, in this process")
    ap.add_argument("--side", choices=["this", "parent"], default="this")
    ap.add_argument("--blobs-only", action="store_true", help="write the plan blobs and stop (no GPU)")
    a = ap.parse_args()
    if a.leg is not None:
        return child(a)
    blobs = os.path.join(ROOT, "profiles", "%s_einsum_blobs" % a.tag)
    if not os.path.exists(os.path.join(blobs, "attention.json")):
        write_blobs(a.tag)
    if a.blobs_only:
        return
    if not a.parent:
        sys.exit("einsum_bench: --parent <built checkout of the parent commit> is needed for the comparison")
    parent_lib = os.path.join(os.path.abspath(a.parent), "ezkl_amd", "libezkl_hip.so")
    if not os.path.exists(parent_lib):
        sys.exit("einsum_bench: %s is not built" % parent_lib)
    for leg in ("dots", "attention"):
        for side in ("this", "parent"):
            env = dict(os.environ)
            env.pop("EZKL_HIP_LIB", None)
            if side == "parent":
                env["EZKL_HIP_LIB"] = parent_lib
            cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--tag", a.tag, "--repeat", str(a.repeat), "--sittings",
                   str(a.sittings), "--leg", leg, "--side", side]
            rc = subprocess.call(cmd, env=env)
            if rc != 0:
                sys.exit("einsum_bench: the %s leg on the %s library ended with status %d: nothing more is started" % (leg, side, rc))
        got = json.load(open(os.path.join(ROOT, "profiles", "%s_einsum.json" % a.tag)))[leg]
        differ = [name for name, e in got["this"].items() if isinstance(e, dict) and e.get("columns") != got["parent"][name].get("columns")]
        if differ:
            sys.exit("einsum_bench: the two libraries wrote different columns for %s" % ", ".join(differ))


if __name__ == "__main__":
    main()
