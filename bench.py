#!/usr/bin/env python3
"""bench.py -- BASELINE.json configs[1]: 2^20-point BN254 G1 MSM + 2^22 Fr NTT microbench per MI355X.

    python bench.py --gpus N --steps K --warmup W [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py --gpus N ...

A "step" is one pass of the hot path over one batch of synthetic input already resident in HBM:
one 2^20-point MSM (uniform scalars) against this rank's slice of a fixed base set -- the metric's
`value` is whole-job MSM points/s.  The 2^22 NTT is timed in a second region of the same K steps and
reported under "extra" (elems/s).  Multi-GPU (weak scaling): every rank owns its own
2^20-point slice; each step ends with an RCCL all_gather of the 64-byte partial points and a host fold,
the only exchange the path has.  NTT columns are independent per rank (no collective).
Rank 0 prints ONE JSON line.

A plain run does only what that line's headline needs: set-up, warm-up, the two timed regions, --dump-outputs,
the line.  --full adds everything else the benchmark measures or checks: per-kernel device times and the
product / copy micro-benchmarks, the side legs (two MSMs in flight, witness-like scalars, inverse and coset
NTTs), the CPU baselines and the end-to-end prove legs, and with N ranks the strong-scaling MSMs and the
sharded proofs.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
T_PROCESS_START = time.time()
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LOG_MSM = 20
LOG_NTT = 22
SEED = 0x657a6b6c
HBM_PEAK_GBS = 8000.0          # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8 TB/s peak
MSM_BYTES_PER_POINT = 96       # 64 B base + 32 B scalar, each read once
NTT_BYTES_PER_ELEM = 64        # read once + write once
CLOCK_WARMUP_MSM = 150         # untimed steps before the contract's --warmup steps (an idle MI355X sits at ~600 MHz): reported as clock_warmup_steps
CLOCK_WARMUP_NTT = 200
NTT_DUMP_SAMPLE = 1 << 18      # --dump-outputs: rows of the 2^22-element NTT output kept (16 MB as float64 words; the whole column would be 256 MB)


def rand_fr(rng, n):
    a = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 61) - 1)     # 253 random bits < r: uniform Montgomery residues
    return a


R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT_R = (1 << 256) % R_MOD


def witness_like_fr(rng, n):
    """SURVEY.md §8(d) / BASELINE.md §3 distribution (W): 70 % small signed values (|x| < 2^15 through integer_rep_to_felt,
    /root/reference/src/fieldutils.rs:9-17), 20 % zero, 10 % uniform -- Montgomery residues, what an advice column holds"""
    out = rand_fr(rng, n)
    kind = rng.random(n)
    lo = -(1 << 15) + 1
    small = rng.integers(lo, 1 << 15, size=n)
    table = np.frombuffer(b"".join(((v % R_MOD) * MONT_R % R_MOD).to_bytes(32, "little") for v in range(lo, 1 << 15)), np.uint64).reshape(-1, 4)
    is_small = kind < 0.7
    out[is_small] = table[small[is_small] - lo]
    out[(kind >= 0.7) & (kind < 0.9)] = 0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true", help="also every figure and check beyond the headline (see the module docstring); a plain run "
                    "is set-up, warm-up, the two timed regions and the line")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: no CPU baselines and no prove legs")
    ap.add_argument("--no-side-legs", action="store_true", help="with --full: no two-in-flight, witness-like, inverse / coset legs")
    ap.add_argument("--with-batch", action="store_true", help="also time the pipelined 4-column batch commit (extra.msm_batch4_*)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo only for 1-GPU plumbing tests)")
    ap.add_argument("--share-device", action="store_true", help="testing only: every rank uses GPU 0")
    ap.add_argument("--dump-outputs", metavar="DIR", help="rank 0 writes what the last timed step of each region returned to DIR/<name>.npy "
                    "(float64; every 254-bit value as its eight 32-bit little-endian words, exact): msm_result (2, 8) = the affine point x, y; "
                    "ntt_sample (%d, 8) = a fixed, seeded sample of the transformed column, rows in ascending index order" % NTT_DUMP_SAMPLE)
    args = ap.parse_args()

    import torch
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and world > 1:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    # stdout belongs to rank 0's ONE line and to nothing else.  Libraries print at C level into the same pipe (RCCL's five-line banner is
    # buffered by stdio and comes out at process exit, i.e. AFTER the line; gloo notes its connections): file descriptor 1 of every rank is
    # pointed at stderr for the whole run, and rank 0 writes its line to the ORIGINAL stdout at the very end (emit)
    global _LINE_FD
    sys.stdout.flush()
    if rank == 0:
        _LINE_FD = os.dup(1)
    os.dup2(2, 1)
    dist = None
    if args.share_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=dev)
        else:
            dist.init_process_group(backend=args.backend)
            dev = torch.device("cpu")          # gloo moves the 64-byte partials through host memory

    import ezkl_amd
    from ezkl_amd import backend as B
    from ezkl_amd import dist as D
    ezkl_amd.init(local_rank)

    if os.environ.get("EZKL_BENCH_FAIL_RANK") == str(rank):          # test hook: this rank dies before its first collective (tests/test_plonk.py)
        raise SystemExit("bench: rank %d asked to fail (EZKL_BENCH_FAIL_RANK)" % rank)
    n_msm, n_ntt = 1 << LOG_MSM, 1 << LOG_NTT
    rng = np.random.default_rng(SEED + rank)
    # ---- synthetic inputs, resident in HBM before any timed region ----
    bases = B.Bases.generate(SEED, n_msm, first=rank * n_msm)       # this rank's slice of the base set
    scalars = B.DeviceBuffer.from_numpy(rand_fr(rng, n_msm))
    dom = ezkl_amd.EvaluationDomain(2, LOG_NTT)
    col = B.DeviceBuffer.from_numpy(rand_fr(rng, n_ntt))

    def barrier_sync():
        torch.cuda.synchronize()
        ezkl_amd.backend.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    def msm_step():
        part = B.msm_g1_dev(bases, scalars.ptr, n_msm)
        return D.fold_partials(part, dist, dev)

    def ntt_step():
        B.ntt_dev(col.ptr, LOG_NTT, dom.omega)

    # clock warm-up before the W contract warm-up steps: an idle MI355X sits at ~600 MHz (rocm-smi on the bench boxes) and a timed region of
    # K = 20 steps is 30 ms long -- 150 steps (~0.25 s) of the same MSM first, untimed, so that the K steps are measured at the clocks a prover runs at
    # (a fixed COUNT, not a duration: with N ranks every step ends in a collective, so every rank must run the same number of them)
    # These clock warm-up steps are reported in the JSON line (`clock_warmup_steps`), next to the contract's `warmup`.
    for _ in range(CLOCK_WARMUP_MSM):
        msm_step()
    for _ in range(args.warmup):
        msm_step()
    barrier_sync()
    # the kernel times of the K timed steps are read AFTER the region (ezkl_hip_kernel_ms_stats: every step records into an event pair of
    # its own, on the stream the kernels run on), so the timed loop holds nothing but the steps
    # ... and only the event pair the roofline needs is recorded in it (EZKL_HIP_TIMING=kernel: the pair around msm_accumulate_kernel; an event
    # record is a barrier packet with a timestamp, and the second pair -- around the whole chain -- costs ~7 us of a 1.31 ms step:
    # profiles/r05aa_wall_probe.log).  The chain's device time is measured right after the region, over its own few steps.
    B.kernel_ms_stats("msm", reset=True); B.kernel_ms_stats("msm_accumulate", reset=True)
    os.environ["EZKL_HIP_TIMING"] = "kernel"
    t0 = time.perf_counter()
    for _ in range(args.steps):
        result = msm_step()
    barrier_sync()
    t_msm = time.perf_counter() - t0
    os.environ.pop("EZKL_HIP_TIMING", None)
    acc_sum, acc_cnt = B.kernel_ms_stats("msm_accumulate")
    acc_ms = [acc_sum / max(1, acc_cnt)]
    errors = []
    if acc_cnt != args.steps or B.kernel_ms_stats("msm")[1] != 0:      # bookkeeping, never worth the headline line
        errors.append("msm_accumulate event pairs harvested: %d for %d timed steps" % (acc_cnt, args.steps))
    if args.full:
        for _ in range(max(5, args.steps // 2)):        # whole-chain device time (both event pairs recorded): outside the timed region
            msm_step()
        barrier_sync()
        msm_sum, msm_cnt = B.kernel_ms_stats("msm")
        msm_ms = [msm_sum / max(1, msm_cnt)]

    # ... and the same K steps with TWO MSMs in flight (ezkl_hip_msm_g1_start_dev / _finish: step i + 1 is queued before step i is waited for,
    # so the latency-bound sort / reduce kernels and the host tail of one step run under the accumulation of the other -- what a prover's
    # commit phases do with their batches).  Reported beside the headline (roofline.msm_two_in_flight), never as `value`: the headline stays
    # the synchronous step of rounds 1-4.  Single rank only (with N ranks every step ends in the fold's collective).
    t_msm2 = None
    side_legs = args.full and not args.no_side_legs
    if world == 1 and side_legs:
        try:
            tok = B.msm_g1_start_dev(bases, scalars.ptr, n_msm)
            for _ in range(3):
                nxt = B.msm_g1_start_dev(bases, scalars.ptr, n_msm); B.msm_g1_finish(tok); tok = nxt
            B.msm_g1_finish(tok)
            barrier_sync()
            t0 = time.perf_counter()
            tok = B.msm_g1_start_dev(bases, scalars.ptr, n_msm)
            for i in range(args.steps):
                nxt = B.msm_g1_start_dev(bases, scalars.ptr, n_msm) if i + 1 < args.steps else None
                result2 = B.msm_g1_finish(tok)
                tok = nxt
            barrier_sync()
            t_msm2 = time.perf_counter() - t0
            if not (result2 == result).all():
                raise SystemExit("bench: pipelined MSM result differs from the synchronous one")
        except SystemExit:
            raise
        except Exception as e:                          # never lose the headline line to this leg
            t_msm2 = None
            print("bench: two-in-flight leg failed: %r" % (e,), file=sys.stderr)

    # ... and the second scalar distribution of the contract: (W) witness-like scalars -- what the advice
    # columns a prover commits look like.  The same K synchronous steps over the same bases; reported beside the headline
    # (roofline.msm_witness_like), checked against the oracle in the cpu_baseline leg.  Single rank only, like the leg above.
    w_leg = None
    if world == 1 and side_legs:
        try:
            scalars_w = B.DeviceBuffer.from_numpy(witness_like_fr(np.random.default_rng(SEED + 17), n_msm))
            for _ in range(max(3, args.warmup)):
                result_w = B.msm_g1_dev(bases, scalars_w.ptr, n_msm)
            barrier_sync()
            B.kernel_ms_stats("msm_accumulate", reset=True)
            os.environ["EZKL_HIP_TIMING"] = "kernel"
            t0 = time.perf_counter()
            for _ in range(args.steps):
                result_w = B.msm_g1_dev(bases, scalars_w.ptr, n_msm)
            barrier_sync()
            t_w = time.perf_counter() - t0
            os.environ.pop("EZKL_HIP_TIMING", None)
            a_s, a_c = B.kernel_ms_stats("msm_accumulate")
            B.kernel_ms_stats("msm", reset=True)
            for _ in range(5):
                B.msm_g1_dev(bases, scalars_w.ptr, n_msm)
            barrier_sync()
            m_s, m_c = B.kernel_ms_stats("msm")
            w_leg = {"pts_per_s": n_msm * args.steps / t_w, "ms_per_step": t_w / args.steps * 1e3, "accumulate_ms": a_s / max(1, a_c),
                     "device_ms": m_s / max(1, m_c), "distribution": "70 % |x| < 2^15 signed, 20 % zero, 10 % uniform (BASELINE.md §3 W)"}
        except Exception as e:                          # never lose the headline line to this leg
            errors.append("witness-like MSM leg failed: %r" % (e,))

    # the NTT region: K transforms queued stream-ordered on the library stream, as a prover queues them (ezkl_hip_set_async), one
    # barrier + synchronise at the end; the MSM region above is synchronous by nature (every step returns its point to the host)
    for _ in range(CLOCK_WARMUP_NTT):
        ntt_step()
    for _ in range(args.warmup):
        ntt_step()
    barrier_sync()
    B.kernel_ms_stats("ntt", reset=True)
    was_async = B.set_async(True)
    os.environ["EZKL_HIP_TIMING"] = "none"              # no event records inside this region either: the transform's device time is measured right after it
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ntt_step()
    barrier_sync()
    t_ntt = time.perf_counter() - t0
    os.environ.pop("EZKL_HIP_TIMING", None)
    if args.dump_outputs and rank == 0:                 # before the steps below transform the column again
        idx = np.sort(np.random.default_rng(SEED + 1).choice(n_ntt, NTT_DUMP_SAMPLE, replace=False))
        dump_outputs(args.dump_outputs, {"msm_result": _words(result).reshape(2, 8),
                                         "ntt_sample": _words(col.to_numpy(shape=(n_ntt, 4))[idx])})
    if args.full:
        for _ in range(max(5, args.steps // 2)):        # the same transforms with their event pair (HIP events around the three passes)
            ntt_step()
        barrier_sync()
    B.set_async(was_async)
    if args.full:
        ntt_sum, ntt_cnt = B.kernel_ms_stats("ntt")
        ntt_ms = [ntt_sum / max(1, ntt_cnt)]
        if ntt_cnt != max(5, args.steps // 2):
            errors.append("ntt event pairs harvested: %d for %d steps" % (ntt_cnt, max(5, args.steps // 2)))

    # the other two forms BASELINE.md §3 names, on the GPU as on the CPU (cpu_baseline.ntt): the inverse transform (lagrange_to_coeff: omega^-1 and
    # the 1/n scale) and the prover's coset form (coeff_to_extended: 2^20 coefficients, zeta twist, zero-extended to 2^22), queued the same way
    ntt_forms, was_async = {}, None
    try:
        if not side_legs:
            raise StopIteration
        was_async = B.set_async(True)
        os.environ["EZKL_HIP_TIMING"] = "none"
        def timed(f):
            for _ in range(max(3, args.warmup)):
                f()
            barrier_sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                f()
            barrier_sync()
            return (time.perf_counter() - t0) / args.steps
        ntt_forms["inverse_elems_per_s"] = world * n_ntt / timed(lambda: B.ntt_dev(col.ptr, LOG_NTT, dom.omega_inv, inverse=True))
        cos_out = B.DeviceBuffer(n_ntt * 32)
        ntt_forms["coset_2p20_to_2p22_elems_per_s"] = world * n_ntt / timed(lambda: B.coset_ntt_dev(col.ptr, cos_out.ptr, 20, 22))
        cos_out.free()
    except StopIteration:
        pass
    except Exception as e:
        errors.append("inverse / coset NTT legs failed: %r" % (e,))
    finally:
        os.environ.pop("EZKL_HIP_TIMING", None)
        if was_async is not None:
            B.set_async(was_async)

    # batched commit (one prover phase: 4 independent 2^20-point columns per call, pipelined over streams)
    # (kept out of the default run so that rocprofv3's per-kernel averages of `python bench.py` are those of the
    #  single-MSM timed region: overlapped launches have longer individual durations)
    NB = 4
    t_batch, bres = None, None
    if args.with_batch:
        bcols = [scalars] + [B.DeviceBuffer.from_numpy(rand_fr(rng, n_msm)) for _ in range(NB - 1)]
        bptrs = [b.ptr for b in bcols]
        B.msm_g1_batch_dev(bases, bptrs, n_msm)
        barrier_sync()
        t0 = time.perf_counter()
        reps = max(1, args.steps // NB)
        for _ in range(reps):
            bres = B.msm_g1_batch_dev(bases, bptrs, n_msm)
        barrier_sync()
        t_batch = (time.perf_counter() - t0) / (reps * NB)

    if dist is not None:
        t = torch.tensor([t_msm, t_ntt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        t_msm, t_ntt = float(t[0]), float(t[1])

    # N > 1: STRONG scaling of one MSM (BASELINE configs[3]: "MSM sharded across 8"): ONE 2^20-point and ONE 2^22-point MSM whose points
    # are split over the ranks, partials folded after an all_gather of 64 bytes per rank -- next to the weak-scaling headline above.
    strong = None
    if world > 1 and args.full:
        try:
            strong = strong_scaling(world, rank, dist, dev, B, D, torch, args, barrier_sync)
        except Exception as e:                      # never lose the headline line to this leg
            strong = {"error": repr(e)[:200]}

    # N > 1: the end-to-end prove with its MSMs sharded by points across the ranks (BASELINE configs[3]).  Every rank starts a
    # CHILD (tools/prove_bench.py) and the children form their own process group on the next port, so a failure or a hang in
    # this leg can only cost its timeout: the headline line below is printed regardless.
    prove_multi = None
    if world > 1 and args.full and not args.no_cpu_baseline:
        prove_multi = prove_leg_multi(world, rank, local_rank, args)

    if rank == 0:
        acc_avg_ms = float(np.mean(acc_ms))
        achieved = MSM_BYTES_PER_POINT * n_msm / (acc_avg_ms * 1e-3) / 1e9
        out = {
            "metric": "BN254 G1 MSM pts/s (2^20 points per GPU; NTT 2^22 elems/s in extra)",
            "value": world * n_msm * args.steps / t_msm,
            "unit": "pts/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "clock_warmup_steps": {"msm": CLOCK_WARMUP_MSM, "ntt": CLOCK_WARMUP_NTT,
                                   "note": "untimed steps of the same workload BEFORE the `warmup` steps, so that the K timed steps run at the clocks a prover runs at"},
            "ms_per_step": t_msm / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u32x8 (254-bit modular integer, Montgomery)",
            "data": "synthetic",
            "config": {"workload": "configs[1]: standalone 2^20-point BN254 G1 MSM (uniform scalars, try-and-increment bases) "
                                   "+ 2^22 scalar-field NTT per GPU", "msm_points_per_gpu": n_msm, "ntt_elems_per_gpu": n_ntt,
                       "parallelism": "points sharded across %d rank(s); all_gather of 64-B partials + host fold" % world},
            # the accumulate kernel's figures come from the event pairs of the timed region itself, so a plain run keeps them
            "roofline": {"bound": "hbm", "kernel": "msm_accumulate_kernel", "achieved": achieved, "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "avg_launch_ms": acc_avg_ms,
                         # the other half of BASELINE.json's metric: the 2^22-point NTT of the second timed region
                         "ntt": {"metric": "BN254 Fr NTT elems/s (2^22 points per GPU)", "elems_per_s": world * n_ntt * args.steps / t_ntt,
                                 "ms_per_step": t_ntt / args.steps * 1e3,
                                 "steps_queued": "stream-ordered (ezkl_hip_set_async), one synchronise after the K steps; no event records inside the timed region"}},
            "extra": {"ntt_elems_per_s": world * n_ntt * args.steps / t_ntt, "ntt_ms_per_step": t_ntt / args.steps * 1e3,
                      "result_x_limb0": int(result[0])},
        }
        if t_batch is not None:
            out["extra"].update({"msm_batch4_ms_per_msm": t_batch * 1e3, "msm_batch4_pts_per_s_per_gpu": n_msm / t_batch,
                                 "batch_matches_single": bool((bres[0] == B.msm_g1_dev(bases, scalars.ptr, n_msm)).all())})
    if rank == 0 and args.full:
        modmul = B.ubench("modmul")
        modmul29 = B.ubench("modmul29")           # the carry-free radix-2^29 product the MSM kernels use
        copy_bps = B.ubench("copy")
        # HBM traffic per launch of the dominant kernel: PMC counters need their own rocprofv3 passes (the guide: never together with the
        # kernel trace), so bench.py cannot measure them itself; it reports the tracked reduction of those passes WITH its source label
        traffic, traffic_source, ntt_traffic = None, None, None
        tpath = os.path.join(ROOT, "profiles", "pmc_traffic.json")  # PMC passes over THIS workload (tools/pmc_run.sh: the 2^20-point uniform MSM of the timed region)
        if os.path.exists(tpath):
            try:
                tj = json.load(open(tpath))
                # the passes are tied to the kernels they measured: tools/pmc_reduce.py stamps the commit and the SHA-256 of msm.hip / ntt.hip; a
                # figure taken from other kernel sources than the ones this run executes is REFUSED (traffic = null, the reason in traffic_source)
                stamp = tj.get("kernel_sources_sha256") or {}
                label = "profiles/pmc_traffic.json: %s (commit %s)" % (tj.get("source"), tj.get("commit"))
                if stamp.get("msm.hip") == _sha256_of("ezkl_amd/csrc/msm.hip"):
                    traffic, traffic_source = tj.get("msm_accumulate_kernel_bytes_per_launch"), label
                else:
                    traffic_source = "refused: " + label + " was taken over another msm.hip than the one that ran (sha256 %s... vs %s...)" % (
                        str(stamp.get("msm.hip"))[:12], _sha256_of("ezkl_amd/csrc/msm.hip")[:12])
                if stamp.get("ntt.hip") == _sha256_of("ezkl_amd/csrc/ntt.hip"):
                    ntt_traffic = tj.get("ntt_2p22_bytes_per_transform")
            except Exception:
                traffic = None
        ntt_gbs = NTT_BYTES_PER_ELEM * n_ntt / (float(np.mean(ntt_ms)) * 1e-3) / 1e9
        rf = out["roofline"]
        rf.update({"traffic": traffic, "traffic_source": traffic_source,
                   "note": "integer-VALU bound, not HBM bound: see roofline.product_peak (NOTEBOOK.md §roofline)",
                   # what the kernels are actually bound by, measured in this run (ezkl_hip_ubench): 254-bit Montgomery products per second with
                   # every lane issuing the radix-2^29 product and nothing else; and the copy bandwidth this device reaches
                   "product_peak": {"modmul29_per_s": modmul29, "modmul32_per_s": modmul, "hbm_copy_GBs": copy_bps / 1e9},
                   "msm_device_ms": float(np.mean(msm_ms)),
                   "timing_events": "timed region: one HIP event pair per step, around msm_accumulate_kernel (EZKL_HIP_TIMING=kernel); msm_device_ms from steps after the region with both pairs",
                   "msm_witness_like": w_leg,
                   "msm_two_in_flight": ({"pts_per_s": n_msm * args.steps / t_msm2, "ms_per_step": t_msm2 / args.steps * 1e3,
                                          "note": "the same K steps with step i + 1 queued before step i is waited for (ezkl_hip_msm_g1_start_dev / _finish); not the headline"}
                                         if t_msm2 else None)})
        rf["ntt"].update({"device_ms_per_transform": float(np.mean(ntt_ms)), "launches_per_transform": 3, "bound": "hbm", "achieved": ntt_gbs,
                          "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ntt_gbs / HBM_PEAK_GBS, "traffic": ntt_traffic,
                          "inverse_elems_per_s": ntt_forms.get("inverse_elems_per_s"), "coset_2p20_to_2p22_elems_per_s": ntt_forms.get("coset_2p20_to_2p22_elems_per_s")})
        rf["ntt"]["steps_queued"] += ", device_ms_per_transform from steps right after it"
        out["extra"].update({"msm_device_ms": float(np.mean(msm_ms)), "ntt_device_ms": float(np.mean(ntt_ms)), "ntt_achieved_GBs": ntt_gbs,
                             "modmul_per_s": modmul, "modmul29_per_s": modmul29, "hbm_copy_GBs": copy_bps / 1e9})
        if not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(bases, scalars, n_msm, result)
            if w_leg is not None:                        # the (W) result against the oracle on the same input
                from oracle import binding as ob_
                t0 = time.perf_counter()
                same_w = bool((ob_.msm(scalars_w.to_numpy(shape=(n_msm, 4)), bases.download()) == result_w).all())
                out["cpu_baseline"]["witness_like"] = {"value": n_msm / (time.perf_counter() - t0), "unit": "pts/s", "matches_gpu_result": same_w}
                if not same_w:
                    raise SystemExit("bench: GPU MSM result (witness-like scalars) differs from the CPU oracle")
            try:
                out["cpu_baseline"]["ntt"] = cpu_baseline_ntt(B, dom)
            except Exception as e:                       # never lose the headline line to this leg
                out["cpu_baseline"]["ntt"] = {"error": repr(e)[:200]}
            out["prove"] = prove_leg()
            # BASELINE.json's metric leads with "ezkl prove wall-seconds (k = 20 MLP)": that number next to `value`, with the CPU prover of
            # the same run beside it (a CPU restatement on this box's host cores, not halo2) and whether the two proofs are the same bytes
            m20 = out["prove"].get("mlp_k20") or {}
            c20 = m20.get("cold") or {}
            out["prove_seconds_k20_mlp"] = {"gpu": m20.get("prove_seconds_gpu"), "gpu_is": "best of %s warm proofs: SRS, key, window tables and JIT code resident, witness laid out in pinned memory" % len(m20.get("prove_seconds_gpu_runs") or []),
                                            "gpu_runs": m20.get("prove_seconds_gpu_runs"), "gpu_first_of_process": m20.get("first_prove_seconds_gpu"),
                                            # the same proof from the witness handed over as int64 IntegerRep columns (8 B per cell across PCIe, ezkl_prover_create_proof_fmt)
                                            "gpu_integer_rep_advice": (m20.get("integer_rep_advice") or {}).get("prove_seconds_gpu"),
                                            "gpu_integer_rep_advice_same_bytes": (m20.get("integer_rep_advice") or {}).get("same_proof_bytes"),
                                            # the CLI-equivalent one-shot: a FRESH process reads SRS + pk + witness files into HBM, proves once, writes proof.json
                                            "cold": c20.get("cold_seconds"), "cold_first_ever": c20.get("first_ever_cold_seconds"), "cold_stages": c20.get("stages"),
                                            "cold_same_proof_as_warm": c20.get("same_proof_as_warm"),
                                            "cpu": m20.get("prove_seconds_cpu"), "cpu_threads": m20.get("cpu_threads"),
                                            "identical": m20.get("proofs_identical_gpu_cpu"), "verifier_accepts": m20.get("verifier_accepts"),
                                            "unit": "s", "higher_is_better": False, "error": m20.get("error")}
        # the three kernels that dominate the metric's own workload (the k = 20 MLP proof), each against the HBM roof: algorithmic bytes per
        # launch / the launch's HIP-event time measured in THIS run; `traffic` = PMC bytes per launch of the same kernel inside a proof
        # (tools/pmc_prove.sh: counters need their own rocprofv3 passes, so the tracked reduction is reported with its source)
        pk_, pm_ = {}, None
        ppath = os.path.join(ROOT, "profiles", "r06_pmc_prove.json")
        if os.path.exists(ppath):
            try:
                pm_ = json.load(open(ppath))
                st_ = pm_.get("kernel_sources_sha256") or {}
                # per kernel: the figure is kept only if the source file of THAT kernel is the one the PMC passes ran on
                ok_ = {"ntt_pass_kernel": st_.get("ntt.hip") == _sha256_of("ezkl_amd/csrc/ntt.hip"),
                       "msm_accumulate_kernel": st_.get("msm.hip") == _sha256_of("ezkl_amd/csrc/msm.hip")}
                pk_ = {k_: v_ for k_, v_ in pm_.get("kernels", {}).items() if ok_.get(k_, True)}
                if "evalh.hip" in st_ and st_.get("evalh.hip") != _sha256_of("ezkl_amd/csrc/evalh.hip"):
                    pm_ = dict(pm_, evalh_jit_sweep={})
                pm_["source"] = "%s (commit %s)" % (pm_.get("source"), pm_.get("commit"))
            except Exception:
                pm_, pk_ = None, {}
        def rk(kernel, workload, alg_bytes, ms, traffic, extra=None):
            d = {"kernel": kernel, "workload": workload, "bound": "hbm", "algorithmic_bytes_per_launch": alg_bytes, "avg_launch_ms": ms,
                 "achieved": (alg_bytes / (ms * 1e-3) / 1e9) if ms else None, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                 "frac": (alg_bytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if ms else None, "traffic": traffic,
                 "traffic_source": ("profiles/%s: %s" % (os.path.basename(ppath), pm_.get("source"))) if (pm_ and traffic) else None}
            d.update(extra or {})
            # the roof these kernels actually sit under: 254-bit Montgomery products per second against the product peak MEASURED IN THIS
            # RUN (extra.modmul29_per_s: ezkl_hip_ubench, every lane issuing the radix-2^29 product the kernels use, nothing else)
            if ms and d.get("products_per_launch") and modmul29:
                d["valu"] = {"bound": "valu (Montgomery products)", "achieved": d["products_per_launch"] / (ms * 1e-3), "peak": modmul29, "unit": "products/s",
                             "frac": d["products_per_launch"] / (ms * 1e-3) / modmul29}
            return d
        ntt_pass_ms = float(np.mean(ntt_ms)) / 3.0                     # a 2^22 transform is three launches of ntt_pass_kernel
        rks = [rk("ntt_pass_kernel", "one of the three passes of the 2^22-point NTT of the timed region (the transform's 64 B per element, read once + written once, divided over its three launches)",
                  NTT_BYTES_PER_ELEM * n_ntt / 3.0, ntt_pass_ms,
                  (pk_.get("ntt_pass_kernel") or {}).get("bytes_per_launch_mean"),
                  {"note": "traffic: mean over the passes of every transform of a k = 20 MLP proof (2^20- and 2^22-point cosets)",
                   # 22 butterfly stages of n/2 twiddle products + the inter-pass twiddle of 2 of the 3 passes, over three launches
                   "products_per_launch": (LOG_NTT * n_ntt / 2 + 2 * n_ntt) / 3.0})]
        sk = ((out.get("prove") or {}).get("mlp_k20") or {}).get("sweep_kernel")
        if sk:
            rks.append(rk("evalh_jit", "quotient sweep of the k = 20 MLP key: one coset of 2^20 rows, %d columns read + 1 written (32 B each)" % sk["columns"],
                          sk["algorithmic_bytes_per_launch"], sk["avg_launch_ms"], (pm_ or {}).get("evalh_jit_sweep", {}).get("bytes_per_launch_mean"),
                          {"products_per_launch": sk.get("products_per_launch"), "products_per_row": sk.get("products_per_row")}))
        # W = 13 signed-digit windows (NOTEBOOK.md §4.1): n W mixed XYZZ additions of 8M + 2S = 10 products each
        rks.append(rk("msm_accumulate_kernel", "2^20-point MSM of the timed region (96 B per point)", MSM_BYTES_PER_POINT * n_msm, acc_avg_ms, traffic,
                      {"products_per_launch": 13 * n_msm * 10}))
        out["roofline_kernels"] = rks
    if rank == 0:
        if prove_multi is not None:
            out["prove"] = prove_multi
        if strong is not None:
            out["extra"]["msm_strong_scaling"] = strong
        if errors:
            out["errors"] = errors
        emit(out)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


_LINE_FD = None          # rank 0: the process's original stdout (main points fd 1 at stderr for everything else)
LINE_LIMIT = 6000        # the driver's record keeps the last 8 000 characters of stdout: the ONE line must fit with room to spare (round 5's 20 KB line was lost)


def _r(x, sig=5):
    """floats to `sig` significant digits (the line is a record, not a checkpoint); containers recursively"""
    if isinstance(x, float):
        return float("%.*g" % (sig, x)) if x == x and abs(x) != float("inf") else None
    if isinstance(x, str):
        return x if len(x) <= 200 else x[:197] + "..."       # no string of a leg (an error text, a label) may grow the line
    if isinstance(x, dict):
        return {k: _r(v, sig) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_r(v, sig) for v in x]
    return x


def compact_line(full):
    """The ONE JSON line of the contract, cut down to the keys the contract reads -- everything else lives in
    bench_full.json.  Pure function of the full record, so tests/test_bench_line.py can size it from canned records without a GPU."""
    g = lambda d, *ks: ({k: d.get(k) for k in ks if d.get(k) is not None} if isinstance(d, dict) else None)
    rf, cb = full.get("roofline") or {}, full.get("cpu_baseline")
    line = {k: full.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                                     "vs_baseline", "dtype", "data")}
    line["clock_warmup_steps"] = g(full.get("clock_warmup_steps"), "msm", "ntt")
    line["config"] = g(full.get("config"), "workload", "parallelism")
    r = g(rf, "bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_ms", "msm_device_ms")
    if "traffic_source" in rf:                       # the figures from here on are those of a --full run
        r["traffic_source"] = (rf.get("traffic_source") or "")[:100] or None
    r["ntt"] = g(rf.get("ntt"), "elems_per_s", "ms_per_step", "device_ms_per_transform", "launches_per_transform", "achieved", "frac", "traffic",
                 "inverse_elems_per_s", "coset_2p20_to_2p22_elems_per_s")
    for k in ("msm_witness_like", "msm_two_in_flight"):
        if rf.get(k):
            r[k] = g(rf[k], "pts_per_s", "ms_per_step", "accumulate_ms", "device_ms")
    if "product_peak" in rf:
        r["product_peak"] = rf["product_peak"]
    # the kernels of the metric's own workload, one short row each (the long form: bench_full.json roofline_kernels)
    if "roofline_kernels" in full:
        r["kernels"] = [dict(g(k_, "kernel", "avg_launch_ms", "achieved", "frac", "traffic"), valu_frac=(k_.get("valu") or {}).get("frac"))
                        for k_ in full["roofline_kernels"]]
    line["roofline"] = r
    p20 = g(full.get("prove_seconds_k20_mlp"), "gpu", "gpu_first_of_process", "cold", "cpu", "cpu_threads", "identical", "verifier_accepts", "error")
    if cb is not None:
        c = g(cb, "value", "unit", "cores", "kind", "matches_gpu_result")
        c["sample"] = (cb.get("sample") or "")[:110]
        c["witness_like"] = cb.get("witness_like")
        c["ntt"] = g(cb.get("ntt"), "value", "unit", "cores", "inverse_2p22_elems_per_s", "coset_2p20_to_2p22_elems_per_s", "matches_gpu_result", "error")
        if p20:
            c["prove_seconds_k20_mlp"] = p20
        line["cpu_baseline"] = c
    if p20:
        line["prove_seconds_k20_mlp"] = p20
    pr = full.get("prove") or {}
    if "n_gpus" in pr or "rccl_ranks_seen" in pr or ("error" in pr and full.get("n_gpus", 1) > 1):        # N > 1: the sharded proof of configs[3]
        line["rccl_ranks_seen"] = pr.get("rccl_ranks_seen")
        m = g(pr, "n_gpus", "sharding", "rccl_ranks_seen", "prove_seconds_gpu", "all_ranks_same_proof", "verifier_accepts", "exchange_ms_per_proof_max", "error")
        c_ = pr.get("circuit")
        m["circuit"] = str((c_.get("circuit") if isinstance(c_, dict) else c_) or "")[:60]
        for sub in ("mlp_k20", "transformer_k22"):
            if isinstance(pr.get(sub), dict):
                m[sub] = g(pr[sub], "prove_seconds_gpu", "all_ranks_same_proof", "verifier_accepts", "rccl_ranks_seen", "exchange_ms_per_proof_max", "error")
        line["prove_multi"] = m
    else:
        brief = lambda d: g(d, "prove_seconds_gpu", "prove_seconds_cpu", "proofs_identical_gpu_cpu", "verifier_accepts", "hbm_in_use_gib_after_prove",
                            "hbm_pool_high_water_gib", "same_proof_as_resident", "cold_seconds", "error")
        others = {n: brief(pr[n]) for n in ("transformer_k22", "transformer_k22_streamed", "mlp_k22", "conv2d_mnist", "einsum", "mlp") if isinstance(pr.get(n), dict)}
        if others:
            line["prove_other_circuits"] = others
        if pr.get("skipped"):
            line["prove_skipped"] = [str(x)[:60] for x in pr["skipped"]][:6]
    if full.get("rccl_ranks_seen") is not None:
        line["rccl_ranks_seen"] = full["rccl_ranks_seen"]
    ss = (full.get("extra") or {}).get("msm_strong_scaling")
    if ss:
        line["msm_strong_scaling"] = {k: (g(v, "ms_per_msm", "pts_per_s") if isinstance(v, dict) else str(v)[:120]) for k, v in ss.items()}
    if full.get("errors"):
        line["errors"] = [str(e)[:120] for e in full["errors"]][:4]
    line["full_record"] = "bench_full.json"
    line = _r(line)
    text = json.dumps(line, separators=(",", ":"))
    # belt and braces: whatever a leg put into the record, the line that goes out is short
    for drop in ("prove_other_circuits", "msm_strong_scaling", "prove_multi", "prove_skipped"):
        if len(text) <= LINE_LIMIT:
            break
        line.pop(drop, None)
        line.setdefault("dropped_for_size", []).append(drop)
        text = json.dumps(line, separators=(",", ":"))
    return text


def emit(full):
    """rank 0: the full record to bench_full.json (repo root, and gpurun_out/ when that exists so that it travels back from the GPU
    box), the contract's line -- and nothing else -- to stdout"""
    paths = [os.path.join(d, "bench_full.json") for d in (ROOT, os.path.join(ROOT, "gpurun_out")) if os.path.isdir(d)]
    if os.environ.get("EZKL_BENCH_FULL"):                 # ... or exactly where the caller wants it (the tests)
        paths = [os.environ["EZKL_BENCH_FULL"]]
    for path in paths:
        try:
            with open(path, "w") as f:
                json.dump(full, f, indent=1)
        except OSError as e:
            print("bench: could not write %s: %r" % (path, e), file=sys.stderr)
    line = compact_line(full)
    if _LINE_FD is not None:
        os.write(_LINE_FD, (line + "\n").encode())
    else:
        print(line, flush=True)


DUMP_LIMIT_BYTES = 64 << 20


def _words(limbs):
    """u64 limbs -> their 32-bit little-endian words as float64 (exact: every word is below 2^53); the last axis doubles"""
    a = np.ascontiguousarray(limbs, np.uint64)
    return a.view("<u4").reshape(a.shape[:-1] + (2 * a.shape[-1],)).astype(np.float64)


def dump_outputs(dirpath, arrays):
    """--dump-outputs: DIR/<name>.npy per array, so that two builds can be compared output for output on the same seeded inputs"""
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit("bench: --dump-outputs would write %d bytes (limit %d)" % (total, DUMP_LIMIT_BYTES))
    os.makedirs(dirpath, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(dirpath, name + ".npy"), a)


def strong_scaling(world, rank, dist, dev, B, D, torch, args, barrier_sync):
    """one MSM of 2^20 (and 2^22) points split over the ranks: rank r commits points [r n/N, (r+1) n/N), the 64-byte partials are
    all_gathered and folded.  Returns whole-MSM milliseconds and points/s (max over ranks), per size."""
    out = {}
    for logn in (20, 22):
        n = 1 << logn
        lo, hi = D.shard_range(n, rank, world)
        bases = B.Bases.generate(SEED + 7, hi - lo, first=lo)                 # this rank's slice of ONE global base set
        rng = np.random.default_rng(SEED + 100 + logn)                       # the same scalar vector on every rank; each uses its slice
        sc = B.DeviceBuffer.from_numpy(np.ascontiguousarray(rand_fr(rng, n)[lo:hi]))
        step = lambda: D.fold_partials(B.msm_g1_dev(bases, sc.ptr, hi - lo), dist, dev)
        for _ in range(max(1, args.warmup)):
            res = step()
        barrier_sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            res = step()
        barrier_sync()
        t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        ms = float(t[0]) / args.steps * 1e3
        out["2^%d" % logn] = {"ms_per_msm": ms, "pts_per_s": n / (ms * 1e-3), "points_per_rank": hi - lo, "result_x_limb0": int(res[0])}
        bases.free()
    return out


def prove_leg():
    """End-to-end `prove` of ezkl circuits (tools/prove_bench.py, tools/bench_circuits.py) in CHILD processes, so that the per-kernel
    averages rocprofv3 reports for this process stay those of the timed MSM / NTT regions.  Part of the checker leg: each child
    verifies its proof with the oracle's pairing verifier.  The legs run in the order of their weight for BASELINE.json's metric and
    each one only if the run's time budget (EZKL_BENCH_BUDGET_S, default 150 s from process start) still covers its estimated cost, so
    that `python bench.py --full` ends within minutes; what was skipped is listed under "skipped":
      * `mlp_k20`: the metric's own configuration, "ezkl prove wall-seconds (k = 20 MLP)" -- 9 x (Gemm 665 x 665 + bias + ReLU) over the ezkl
        gate set, laid out once and shipped as bench_cache/mlp_k20_s1.npz; warm prove on the GPU, then the same create_proof on the host
        cores (Python host + C oracle kernels, OpenMP) with identical proof bytes;
      * `conv2d_mnist`: BASELINE configs[2], examples/conv2d_mnist/main.rs's Config and layout at k = 17, GPU and CPU;
      * `einsum`: the reference's own criterion bench circuit benches/accum_einsum_matmul.rs raised to k = 20 (BASELINE configs[3]), GPU and
        CPU; with budget left also the COLD one-shot prove (fresh process, SRS + pk files -> HBM -> proof.json);
      * `mlp`: the MLP at k = 17 (BASELINE configs[2]'s size), GPU and CPU."""
    import subprocess
    tool = os.path.join(ROOT, "tools", "prove_bench.py")
    budget = float(os.environ.get("EZKL_BENCH_BUDGET_S", "420"))
    left = lambda: budget - (time.time() - T_PROCESS_START)
    leg_seconds, skipped = {}, []

    def child(name, env_extra, flags, timeout):
        env = dict(os.environ, **env_extra)
        t0 = time.time()
        try:
            r = subprocess.run([sys.executable, tool] + flags, env=env, capture_output=True, text=True, timeout=timeout)
        finally:
            leg_seconds[name] = round(time.time() - t0, 1)
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if not lines:
            raise RuntimeError(r.stderr[-300:])
        return json.loads(lines[-1])

    def pick(j, keys):
        return {a: j.get(a) for a in keys if a in j}

    common = ["circuit", "cold", "prove_seconds_gpu", "prove_seconds_gpu_runs", "first_prove_seconds_gpu", "prove_seconds_cpu", "cpu_threads", "verifier_accepts", "proof_bytes",
              "keygen_seconds_gpu", "cpu_breakdown_seconds", "hbm_in_use_gib_after_prove", "hbm_pool_high_water_gib", "host_peak_rss_gib"]

    def shape(j, extra=()):
        d = pick(j, common + list(extra))
        d["proofs_identical_gpu_cpu"] = j.get("proofs_identical")
        d["breakdown_seconds"] = j.get("prove_breakdown_seconds")
        return d

    out = {}
    # 1. the metric's own configuration.  Estimated cost on a fresh box: ~25 s for the GPU side (imports, SRS, key generation, 1 + 3 proofs, the
    #    Python verifier), ~60 s more with the CPU prover (its key generation + one proof on 16 threads)
    try:
        if os.environ.get("EZKL_BENCH_MLP20", "1") != "0":
            with_cpu = os.environ.get("EZKL_BENCH_MLP20_CPU", "1") != "0" and left() > 95
            # + the cold one-shot of the metric's own circuit (artefact files -> a fresh process -> proof.json): ~30 s more
            with_cold = os.environ.get("EZKL_BENCH_MLP20_COLD", "1") != "0" and left() > (95 if with_cpu else 25) + 40
            j = child("mlp_k20", {"CIRCUIT": "mlp", "K": "20", "REPS": "3"}, ["--pinned", "--integer-rep"] + (["--cpu"] if with_cpu else []) + (["--cold"] if with_cold else []), 900)
            out["mlp_k20"] = shape(j, ["sweep_kernel", "integer_rep_advice"])
            if not with_cpu:
                skipped.append("mlp_k20 CPU prover")
            if not with_cold:
                skipped.append("mlp_k20 cold one-shot")
    except Exception as e:
        out["mlp_k20"] = {"error": repr(e)[:300]}
    # 1b. BASELINE configs[4]'s size (nanoGPT-tiny, k = 22, SRS 2^22; /root/reference/tests/integration_tests.rs:172-181) as a transformer-SHAPED
    #     SURROGATE (ezkl_layout.TransformerSurrogateCircuit -- NOT the nanoGPT graph, whose layout is ezkl's Model::layout): three static lookup
    #     tables (softmax / layer norm), a dynamic lookup, a shuffle, a Freivalds einsum with second-phase advice and two challenges, degree 6
    #     -> the extended domain is 2^25.  One unit is laid out and tiled with numpy: a FULL circuit in ~10 s, no laid-out file in the
    #     repository.  Two children: the key resident (210 GiB of columns at the peak) and the one-GPU degraded mode EZKL_KEY_COSETS=recompute
    #     (72 GiB: the sweep rebuilds one coset at a time) -- same proof bytes.  ~45 s + ~35 s.  EZKL_BENCH_K22=0 skips, =1 forces;
    #     EZKL_BENCH_K22=mlp runs the round-5 MLP surrogate instead (needs bench_cache/mlp_k22_s1_blocks5_fill25.npz, no longer shipped).
    k22 = os.environ.get("EZKL_BENCH_K22", "auto")
    if k22 == "mlp":
        try:
            j = child("mlp_k22", {"CIRCUIT": "mlp", "K": "22", "MLP_BLOCKS": "5", "MLP_FILL": os.environ.get("EZKL_BENCH_K22_FILL", "25"), "REPS": "2"}, ["--pinned"], 7200)
            out["mlp_k22"] = dict(shape(j), label="MLP surrogate of configs[4] (k = 22, 30 advice columns, SRS 2^22): the size, not the nanoGPT graph")
        except Exception as e:
            out["mlp_k22"] = {"error": repr(e)[:300]}
    elif k22 == "1" or (k22 == "auto" and left() > 110):
        try:
            j = child("transformer_k22", {"CIRCUIT": "transformer", "K": "22", "REPS": "2", "EZKL_KEY_COSETS": "auto"}, [], 1200)
            out["transformer_k22"] = dict(shape(j, ["proof_sha256"]), label="transformer-shaped surrogate of configs[4] (k = 22, ext 2^25, 28 lookups, second-phase advice): not the nanoGPT graph")
            if k22 == "1" or left() > 70:
                js = child("transformer_k22_streamed", {"CIRCUIT": "transformer", "K": "22", "REPS": "1", "EZKL_KEY_COSETS": "recompute"}, [], 1200)
                out["transformer_k22_streamed"] = dict(shape(js, ["proof_sha256"]), label="the same proof with the key streamed (EZKL_KEY_COSETS=recompute)",
                                                       same_proof_as_resident=js.get("proof_sha256") == j.get("proof_sha256"))
            else:
                skipped.append("transformer_k22 streamed key")
        except Exception as e:
            out.setdefault("transformer_k22", {})["error"] = repr(e)[:300]
    else:
        skipped.append("transformer_k22 (surrogate of configs[4])")
    # 2. BASELINE configs[2] as the reference states it: examples/conv2d_mnist at k = 17 (~12 s with its CPU prover)
    if left() > 20:
        try:
            out["conv2d_mnist"] = shape(child("conv2d_mnist", {"CIRCUIT": "conv", "K": "17"}, ["--cpu", "--pinned"], 300))
        except Exception as e:
            out["conv2d_mnist"] = {"error": repr(e)[:300]}
    else:
        skipped.append("conv2d_mnist")
    # 3. BASELINE configs[3]: the reference's bench circuit at k = 20 (~30 s with the CPU prover; the cold one-shot adds ~25 s: it writes
    #    4 GB of artefacts and starts two fresh processes)
    k_e = os.environ.get("EZKL_BENCH_EINSUM_K", "20")
    if left() > 45:
        try:
            cold = os.environ.get("EZKL_BENCH_COLD", "auto")
            with_cold = cold == "1" or (cold == "auto" and left() > 75 + 120)      # the MLP legs (k = 20 cold above, k = 22 below) come first
            j = child("einsum", {"CIRCUIT": "einsum", "K": k_e}, ["--cpu"] + (["--cold"] if with_cold else []), 600)
            out["einsum"] = shape(j)
            out["einsum"].update({"cold_seconds": (j.get("cold") or {}).get("cold_seconds"), "cold": j.get("cold"), "cpu_prover": j.get("cpu_prover"),
                                  "host": "libezkl_prover.so (C++) over the C ABI; ChaCha20 randomness expanded on the device"})
            if not with_cold:
                skipped.append("einsum cold one-shot")
        except Exception as e:
            out["einsum"] = {"error": repr(e)[:300]}
    else:
        skipped.append("einsum k=%s" % k_e)
    # 4. the MLP at k = 17 (~15 s)
    if left() > 25:
        try:
            out["mlp"] = shape(child("mlp_k17", {"CIRCUIT": "mlp", "K": os.environ.get("EZKL_BENCH_MLP_K", "17")}, ["--cpu", "--pinned"], 300))
        except Exception as e:
            out["mlp"] = {"error": repr(e)[:300]}
    else:
        skipped.append("mlp k=17")
    out["leg_seconds"] = leg_seconds
    out["skipped"] = skipped
    out["budget_seconds"] = budget
    return out


def prove_leg_multi(world, rank, local_rank, args):
    """BASELINE configs[3]: the reference's accum_einsum_matmul bench circuit at k = 20 proved by libezkl_prover.so across `world` GPUs --
    every rank holds the complete SRS (288 GB of HBM: base sets + window tables are < 2 GB); every witness column is transformed and
    committed by ONE rank, lookup / permutation arguments run on their owner, the quotient sweep is divided into row units fed by one
    all-to-all, h is all_gathered in place, SHPLONK travels as two 64-byte folds -- through the library's own RCCL communicator
    (csrc/comm.hip).  Every rank emits the same proof bytes; rank 0 verifies them.  Runs in child processes
    (EZKL_BENCH_MULTI_CIRCUIT=mlp selects another circuit)."""
    circuit = os.environ.get("EZKL_BENCH_MULTI_CIRCUIT", "einsum")
    out = _prove_multi_one(world, rank, local_rank, args, circuit, os.environ.get("EZKL_BENCH_MULTI_K", "20"), 1)
    # ... and the north star's k = 20 MLP circuit the same way (laid out ONCE: the first rank to take the lock writes
    # bench_cache/mlp_k20_s1.npz, the others read it -- tools/bench_circuits.py)
    # (skipped when the first leg failed: the same communicator would fail or hang again, and every rank must take the same branch --
    # rank 0 alone knows the outcome, so it is shared through the ranks' process group)
    ok = _all_ranks_agree(world, rank, out is not None and "error" not in out)
    if ok and circuit == "einsum" and os.environ.get("EZKL_BENCH_MULTI_MLP20", "1") != "0":
        m = _prove_multi_one(world, rank, local_rank, args, "mlp", "20", 2)
        if rank == 0 and out is not None:
            out["mlp_k20"] = m
        ok = _all_ranks_agree(world, rank, m is not None and "error" not in m)
    # ... and BASELINE configs[4]: "k = 22, SRS 2^22, 8 x MI355X with NTT + MSM both sharded" -- the transformer-shaped surrogate (every rank
    # builds the same tiled circuit in ~10 s; degree 6: eight cosets of the extended domain 2^25, one per rank at N = 8; every witness column
    # transformed and committed by its owner, the key's cosets by owner).  EZKL_BENCH_MULTI_K22=<k> picks another size (the one-device tests), 0 skips.
    k22 = os.environ.get("EZKL_BENCH_MULTI_K22", "22")
    if ok and circuit == "einsum" and k22 != "0":
        t_ = _prove_multi_one(world, rank, local_rank, args, "transformer", k22, 3)
        if rank == 0 and out is not None:
            out["transformer_k22"] = t_
    return out


def _all_ranks_agree(world, rank, flag_rank0):
    import torch
    import torch.distributed as dist
    if world == 1 or not dist.is_initialized():
        return bool(flag_rank0)
    dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
    t = torch.tensor([1 if (flag_rank0 or rank != 0) else 0], dtype=torch.int32, device=dev)
    dist.broadcast(t, src=0)
    return bool(int(t.item()))


def _prove_multi_one(world, rank, local_rank, args, circuit, k, port_offset):
    """tools/prove_multi.py in a child per rank: libezkl_prover.so with columns and arguments BY OWNER (NTTs by columns, lookup / permutation
    arguments by owner, the sweep in row units fed by one all-to-all, SHPLONK as per-rank partial sums); EZKL_BENCH_MULTI_MODE=replicated
    selects the round-2 mode (commit batches by columns, everything else replicated)"""
    import subprocess
    env = dict(os.environ, K=k, CIRCUIT=circuit, REPS="3", MASTER_ADDR=os.environ.get("MASTER_ADDR", "127.0.0.1"),
               MASTER_PORT=str(int(os.environ.get("MASTER_PORT", "29500")) + port_offset), WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK=str(local_rank))
    for k_ in list(env):                       # the children rendezvous on their own: no torchrun agent store behind the new port
        if k_.startswith("TORCHELASTIC_") or k_ in ("GROUP_RANK", "ROLE_RANK", "ROLE_NAME", "LOCAL_WORLD_SIZE", "GROUP_WORLD_SIZE", "ROLE_WORLD_SIZE",
                                                      "TORCH_NCCL_ASYNC_ERROR_HANDLING"):
            env.pop(k_)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "prove_multi.py"), "--pinned"]
    if args.backend != "nccl":
        cmd.append("--gloo")
    if args.share_device:
        cmd.append("--share-device")
    if os.environ.get("EZKL_BENCH_MULTI_MODE") == "replicated":
        cmd.append("--replicated")
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=int(os.environ.get("EZKL_BENCH_PROVE_TIMEOUT", "300" if circuit == "einsum" else "600")))  # the MLP may have to be laid out first; the k = 22 surrogate is built and keyed per rank
        if rank != 0:
            return None
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if not lines:
            raise RuntimeError(r.stderr[-300:])
        j = json.loads(lines[-1])
        return {"circuit": j["circuit"], "n_gpus": j["n_gpus"], "host": "libezkl_prover.so (C++) over the C ABI", "sharding": j["mode"], "collectives": j["collectives"],
                "rccl_ranks_seen": min(p_["stats"].get("rccl_ranks_seen", 0) for p_ in j["per_rank"]),
                "exchange_ms_per_proof_max": max(p_["stats"].get("exchange_ms_per_proof", 0) for p_ in j["per_rank"]),
                "exchange_bytes_sent_per_proof_max": max(p_["stats"].get("exchange_bytes_sent_per_proof", 0) for p_ in j["per_rank"]),
                "nccl_sends_per_proof_max": max(p_["stats"].get("nccl_sends_per_proof", 0) for p_ in j["per_rank"]),
                "sharded_sweeps": min(p_["sharded_sweeps"] for p_ in j["per_rank"]), "per_rank": j["per_rank"],
                "prove_seconds_gpu": j["prove_seconds_gpu"], "prove_seconds_gpu_runs": j.get("prove_seconds_gpu_runs"), "all_ranks_same_proof": j["all_ranks_same_proof"],
                "verifier_accepts": j["verifier_accepts"], "proof_bytes": j["proof_bytes"], "proof_sha256": j.get("proof_sha256"),
                "keygen_seconds_gpu": j["keygen_seconds_gpu"], "breakdown_seconds": j["prove_breakdown_seconds"]}
    except Exception as e:
        return {"error": repr(e)[:300]} if rank == 0 else None


def _sha256_of(rel):
    import hashlib
    try:
        return hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest()
    except OSError:
        return "missing"


def cpu_baseline_ntt(B, dom):
    """BASELINE.md §3's CPU side of the NTT half of the metric: the C oracle (oracle/oracle.c: the restatement of halo2curves' best_fft and of
    the EvaluationDomain wrappers, OpenMP) on the host cores -- one forward 2^22-point transform, one inverse (lagrange_to_coeff) and the
    prover's coset form (coeff_to_extended 2^20 -> 2^22), best of 2 each (~10 s of CPU work); the forward transform is also the last parity check
    of the NTT region (GPU transform of the same column == oracle's)."""
    from oracle import binding as ob
    rng = np.random.default_rng(SEED + 99)
    a = rand_fr(rng, 1 << LOG_NTT)
    w = ob.omega(LOG_NTT)
    ob.fft(a[: 1 << 12].copy(), 12, ob.omega(12))               # start the OpenMP pool
    def best(f, reps=2):
        ts, r = [], None
        for _ in range(reps):
            t0 = time.perf_counter(); r = f(); ts.append(time.perf_counter() - t0)
        return min(ts), r
    t_fwd, want = best(lambda: ob.fft(a, LOG_NTT, w))
    d = B.DeviceBuffer.from_numpy(a)
    B.ntt_dev(d.ptr, LOG_NTT, dom.omega)
    if not (d.to_numpy(shape=(1 << LOG_NTT, 4)) == want).all():
        raise SystemExit("bench: GPU NTT result differs from the CPU oracle")
    t_inv, _ = best(lambda: ob.lagrange_to_coeff(a, LOG_NTT))
    t_cos, _ = best(lambda: ob.coeff_to_extended(a[: 1 << 20], 20, 22))
    n = 1 << LOG_NTT
    return {"value": n / t_fwd, "unit": "elems/s", "cores": ob.num_threads(), "kind": "port",
            "sample": "one forward 2^22-point transform of the timed workload's size, best of 2 (%.2f s each)" % t_fwd,
            "inverse_2p22_elems_per_s": n / t_inv, "coset_2p20_to_2p22_elems_per_s": n / t_cos,
            "seconds": {"forward_2p22": t_fwd, "lagrange_to_coeff_2p22": t_inv, "coeff_to_extended_2p20_to_2p22": t_cos},
            "matches_gpu_result": True}


def cpu_baseline(bases, scalars, n, gpu_result):
    """The C oracle (oracle/oracle.c: the CPU restatement of halo2curves' Pippenger, NOT halo2curves) timed on
    the host cores of this box on the same 2^20-point input; also the last parity check of the run."""
    from oracle import binding as ob
    pts = bases.download()
    sc = scalars.to_numpy(shape=(n, 4))
    ob.msm(sc[:4096], pts[:4096])              # start the OpenMP pool outside the timed calls
    times = []
    for _ in range(3):                         # ~20 s of CPU work in total on 16 threads
        t0 = time.perf_counter()
        want = ob.msm(sc, pts)
        times.append(time.perf_counter() - t0)
        if not (want == gpu_result).all():
            raise SystemExit("bench: GPU MSM result differs from the CPU oracle")
    dt = min(times)
    return {"value": n / dt, "unit": "pts/s", "cores": ob.num_threads(), "kind": "port",
            "sample": "the full 2^20-point MSM of the timed workload, best of 3 (%.2f s of CPU wall each, %d threads)" % (dt, ob.num_threads()),
            "matches_gpu_result": True}


if __name__ == "__main__":
    main()
