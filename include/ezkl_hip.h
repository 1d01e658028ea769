/*
 * ezkl_hip.h -- C ABI of libezkl_hip.so, the MI355X (gfx950) backend for the `ezkl prove` hot path.
 *
 * This is the drop-in boundary of SURVEY.md §8(b): the functions below are what the halo2 fork's
 * `halo2_proofs::icicle` glue asks of the icicle runtime today (gate: cargo feature `gpu-accelerated`,
 * /root/reference/Cargo.toml:259; runtime gate ENABLE_ICICLE_GPU / ICICLE_SMALL_K,
 * /root/reference/README.md:106-122; device selection /root/reference/src/execute.rs:84-97).
 * Plain pointers and sizes only; no C++/torch types; never throws or unwinds across the boundary.
 *
 * Representation contract (fixture-verified, SURVEY.md §8(b,c)):
 *   Fr / Fq element : 32 bytes, 4 x u64 little-endian limbs, Montgomery form (R = 2^256), fully reduced
 *   G1 affine point : 64 bytes, x || y (Fq), identity encoded as (0,0)  -- the raw-bytes SRS layout
 * Results are canonical (fully reduced, affine), so equality with the CPU prover is byte equality.
 *
 * Threading: every entry point is callable from any host thread (halo2 calls from rayon workers);
 * the library lazily initialises on first use (the Python bindings never call set_device(),
 * /root/reference/src/bindings/python.rs:1056-1075) and serialises per device internally.
 */
#ifndef EZKL_HIP_H
#define EZKL_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (0 = ok, negative = error; see ezkl_hip_strerror) ---- */
#define EZKL_OK 0
#define EZKL_ERR_NO_DEVICE (-1)   /* no HIP device visible: the product path fails loudly, no CPU fallback */
#define EZKL_ERR_HIP (-2)         /* a HIP runtime call failed; ezkl_hip_last_hip_error() has the code */
#define EZKL_ERR_INVALID (-3)     /* bad argument (null pointer, size out of range, bad program) */
#define EZKL_ERR_NOMEM (-4)
#define EZKL_ERR_UNSUPPORTED (-5)
#define EZKL_ERR_TIMEOUT (-7)     /* a collective did not complete within EZKL_COMM_TIMEOUT_S seconds (comm.hip's watchdog): the communicator is aborted */
#define EZKL_ERR_BUSY (-6)        /* the calling thread already holds every slot of a bounded resource (ezkl_hip_msm_g1_start_dev: four per context) */


/* ---- environment: every variable libezkl_hip.so and libezkl_prover.so read, in ONE place (round 6: the A/B switches of rounds 3-5 --
 *      EZKL_MSM_PREFETCH / LEAN / FETCH_ALWAYS / UNPACK_FIRST / RESET_ZZ / COOP / ZEROCOPY / ORDER_ALWAYS / NO_TAPER / FIXUP_TREE /
 *      DEBUG_PLANES, EZKL_NTT_LOAD_ALWAYS / SKIP_UNIT2, EZKL_PROVER_MERGED_COMMITS -- are gone from the sources; their measurements are in profiles/).  All are read
 *      in-process (getenv); unset = the default.  A fork exposes the first group, the rest is for whoever works on the library.
 *
 *  gate and modes (what a deployment sets)
 *   ENABLE_HIP_GPU            unset   the runtime gate, as ENABLE_ICICLE_GPU: ezkl_hip_enabled(k) is 0 without it
 *   HIP_SMALL_K               8       circuits with k <= this stay on the CPU prover, as ICICLE_SMALL_K
 *   LOCAL_RANK                unset   ezkl_hip_init(-1): one context on this device instead of one per visible device
 *   EZKL_KEY_COSETS           auto    auto | resident | recompute: how a proving key is held (ezkl_prover.h: the streamed / degraded mode)
 *   EZKL_PROVER_SKIP_FIT_CHECK unset  1: no up-front HBM fit check at keygen / key load
 *   EZKL_COMM_TIMEOUT_S       120     watchdog of every collective (0: none): EZKL_ERR_TIMEOUT instead of a hang
 *   EZKL_COMM_SELFTEST        1       0: ezkl_hip_comm_init does not run ezkl_hip_comm_selftest (same value on every rank)
 *   EZKL_COMM_SLAB_MB         128     bytes per peer and round of the packed all-to-all (same value on every rank)
 *   EZKL_HIP_CACHE_DIR        ~/.cache/ezkl_hip   where compiled sweep kernels are kept ("off": nowhere)
 *   EZKL_HIP_POOL_CAP_GB      25 % of the device, at least what is live x 1.5   floor of the column pool's footprint bound
 *   EZKL_PK_READ_THREADS      4       reader threads of ezkl_prover_pk_read_file
 *   EZKL_SRS_CHECK            points  points | full | off: (Python bindings, execute.py) what the SRS loaders check before a point set is
 *                                     used -- every point that will be used (ezkl_hip_bases_check), also the file's structure, or nothing
 *   EZKL_HIP_LIB / EZKL_PROVER_LIB    (Python bindings) another build of the two libraries
 *  measurement
 *   EZKL_HIP_TIMING           all     all | kernel | none: which HIP event pairs a timed call records (ezkl_hip_kernel_ms_stats)
 *   EZKL_MSM_HOST_TIMING, EZKL_PROVER_KEYGEN_TIMING     host-side stage times on stderr
 *   EZKL_HIP_DEBUG, EZKL_MSM_DEBUG, EZKL_HIP_JIT_DEBUG, EZKL_HIP_JIT_DUMP=<file>     diagnostics on stderr / the generated sweep source
 *  tuning knobs whose defaults are the measured optimum (NOTEBOOK.md §4; tools/ab.sh sweeps them)
 *   EZKL_MSM_SLOTS 4 | EZKL_MSM_GROUP / _SMALL 6 / _BIG 4 | EZKL_MSM_L (device-chosen) | EZKL_MSM_LMIN 8 | EZKL_MSM_SPAN 16 | EZKL_MSM_E 8
 *     read at every call: EZKL_MSM_GROUP, EZKL_MSM_L, EZKL_MSM_E;  once per process: EZKL_MSM_SLOTS, _GROUP_SMALL, _GROUP_BIG, _LMIN, _SPAN
 *     (msm.hip: msm_tuning and msm_slots_init read them all; a value outside the accepted range keeps the default)
 *   EZKL_NTT_MAXR 8 (9 / 10: 2048- / 4096-element tiles) | EZKL_PROVER_SWEEP_TERMS 0 | EZKL_PROVER_SWEEP_INSTRS 640
 *  comparison switches kept because tests or the multi-rank fallbacks use them
 *   EZKL_EVALH_MODE=interp (the sweep interpreter instead of the JIT kernel), EZKL_EVALH_NO_SCHEDULE, EZKL_COMM_UNPACKED=1 (one send / recv per
 *   segment), EZKL_COMM_SELF_VIA_RCCL=1 (world 1 through the wire format), EZKL_GATHER_HOST, EZKL_MSM_SERIAL_CALLS, EZKL_HIP_POOL_SYNC,
 *   EZKL_PROVER_SYNC_CALLS, EZKL_PROVER_NO_EARLY_RANDOM, EZKL_PROVER_NO_SUM_SCATTER,
 *   EZKL_PROVER_ASSUME_FREE_GIB=<x> (test hook of the fit check) ---- */

typedef struct ezkl_bases_s* ezkl_bases_t;     /* device-resident G1 base set (SRS g or g_lagrange) */

/* ---- device management: replaces icicle try_load_and_set_backend_device("CUDA") + warmup(),
 *      /root/reference/src/execute.rs:88-95 ---- */
/* ezkl_hip_init(device >= 0): one context on that device.  ezkl_hip_init(-1): ALL visible devices, one context per device (context i
 * on device i) -- `ezkl prove` is one process (src/execute.rs:1575-1627) -- unless LOCAL_RANK is set (a launcher started one process
 * per GPU): then one context on device LOCAL_RANK.  Idempotent, thread-safe. */
int ezkl_hip_init(int device);
/* ---- contexts: single-process multi-GPU ----
 * A context = one device + everything the library keeps for it (streams, scratch arenas, MSM window tables and slots, NTT plans,
 * JIT modules, the column pool), behind its own lock.  Every host thread works on the context it bound itself to
 * (ezkl_hip_set_context; new threads start on context 0), so N threads drive N GPUs concurrently and handles (bases, device pointers,
 * upload phases, batches) belong to the context they were made on.  ezkl_hip_contexts_configure(n, devices) sets the table
 * explicitly BEFORE first use -- several contexts may name the same device (how the multi-device prover is tested on a one-GPU box).
 * ezkl_hip_memcpy_peer: device-to-device copy INTO the calling thread's context (dst_context must be it) from another context
 * (hipMemcpyPeerAsync across devices), ordered on the calling context's library stream; the source may be reused once this context has
 * synchronised (ezkl_hip_synchronize). */
int ezkl_hip_contexts_configure(int n_contexts, const int* devices);
int ezkl_hip_context_count(void);
int ezkl_hip_set_context(int index);
int ezkl_hip_context_device(int index);                /* device ordinal of a context, -1 if out of range */
int ezkl_hip_memcpy_peer(void* dst_dev, int dst_context, const void* src_dev, int src_context, size_t bytes);
int ezkl_hip_warmup(void);
int ezkl_hip_device_count(void);
int ezkl_hip_mem_info(size_t* free_bytes, size_t* total_bytes);   /* hipMemGetInfo of the calling context's device */
/* The column pool of the calling context (ezkl_hip_malloc / ezkl_hip_free recycle blocks by exact size; icicle's DeviceVec allocations
 * behind the reference's wrappers play this role).  live + parked bytes are held to max(25 % of the device / contexts sharing it,
 * 1.5 x the high-water mark of the live bytes); least recently used size classes are released first; an out-of-memory hipMalloc
 * releases what every idle context of the device has parked and retries once.  EZKL_HIP_POOL_CAP_GB overrides the 25 %.
 * ezkl_hip_pool_stats: out[0] = bytes handed out now, out[1] = their high-water mark, out[2] = bytes parked, out[3] = the bound.
 * ezkl_hip_pool_trim: release every parked block of the calling context and forget the high-water mark. */
int ezkl_hip_pool_stats(size_t out[4]);
int ezkl_hip_pool_trim(void);
int ezkl_hip_synchronize(void);
/* caller streams for the `stream` arguments below (a hipStream_t created by the caller works just as well; these exist so
 * that a client of this header alone can use the stream-ordered mode): work queued on one is asynchronous */
int ezkl_hip_stream_create(void** out_stream);
int ezkl_hip_stream_synchronize(void* stream);
int ezkl_hip_stream_destroy(void* stream);
/* A second stream owned by the calling thread's context, created on first use and alive as long as the context: creating and
 * destroying a HIP stream costs ~2 ms each (measured, profiles/r03v_hosttrace.txt), which a per-proof auxiliary stream would pay in
 * every proof.  Not to be destroyed by the caller; one per context, so two concurrent users of one context must agree on it. */
int ezkl_hip_context_stream(void** out_stream);
/* Asynchronous library stream.  By default a call with stream == NULL returns when its work is done.  A host that issues hundreds of
 * small device-only calls per proof (vec ops, scans, NTTs, inversions: the lookup / permutation helper chains) pays a host round trip
 * for each; ezkl_hip_set_async(1, &prev) makes those calls return as soon as they are queued on the library stream -- still in order
 * with each other.  Entry points that return host data (MSMs, eval_poly*, lookup_multiplicity, memcpy_d2h) or borrow host memory
 * (memcpy_h2d, eval_h_dev, divide_by_vanishing) keep synchronising by themselves.  ezkl_hip_set_async(0, ..) drains the stream.
 * The mode is a property of the CALLING THREAD: concurrent provers on other threads, and unrelated callers, keep their own setting.
 * ezkl_hip_stream_wait_library(s): work queued on the caller stream s from now on waits for everything queued on the library
 * stream so far (a column produced by library-stream calls, consumed on s). */
int ezkl_hip_set_async(int on, int* previous);
int ezkl_hip_stream_wait_library(void* stream);
const char* ezkl_hip_strerror(int code);
int ezkl_hip_last_hip_error(void);
const char* ezkl_hip_version(void);
/* The runtime gate, in one place for every host language: 1 if the environment variable ENABLE_HIP_GPU is set (to anything:
 * like ENABLE_ICICLE_GPU it is disabled by unsetting it, /root/reference/README.md:106-122) and k > HIP_SMALL_K (default 8, the
 * role of ICICLE_SMALL_K: below the cutoff the caller keeps its CPU path), else 0.  Touches no device. */
int ezkl_hip_enabled(uint32_t k);

/* ---- raw device memory for resident columns (library-owned until freed) ----
 * Freed blocks are recycled by size without returning to the driver (no implicit device synchronisation, unlike hipFree):
 * a block that was used on a CALLER stream must not be freed before that stream has been synchronised.  Blocks only
 * touched through stream = NULL calls are always safe to free. */
int ezkl_hip_malloc(void** dptr, size_t bytes);
int ezkl_hip_free(void* dptr);
int ezkl_hip_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes);
/* page-locked host memory for columns that will be uploaded (the witness: A x 2^k x 32 B per proof).  Copies from it run
 * without the runtime's pageable staging step; a fork would allocate the advice / instance vectors that synthesize() fills
 * from here.  (On the measured box the blocking pageable path was already as fast: 14 x 32 MiB in ~10 ms either way.) */
int ezkl_hip_host_malloc(void** host_ptr, size_t bytes);
int ezkl_hip_host_free(void* host_ptr);
int ezkl_hip_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes);

/* ---- MSM: replaces ParamsKZG::commit / commit_lagrange -> halo2curves::msm (CPU) / icicle msm (GPU);
 *      in-tree call site /root/reference/src/circuit/modules/polycommit.rs:71 ---- */
/* bases: n affine points, host pointer, copied to HBM once (SRS load time, src/pfsys/srs.rs:40-47) */
int ezkl_hip_bases_upload(const void* affine_pts, size_t n, ezkl_bases_t* out_handle);
/* start the per-base-set precompute (the window tables of msm.hip, ~55 ms for 2^20 points) on a library stream WITHOUT waiting: a
 * one-shot `prove` (src/execute.rs:1575-1627) uploads the SRS, calls this, and reads the proving key while the tables are built.
 * Optional: the first MSM on a base set builds them itself (blocking) when this was not called.  The icicle build does the analogous
 * work at ParamsKZG::read time. */
int ezkl_hip_bases_prepare(ezkl_bases_t h);
int ezkl_hip_bases_free(ezkl_bases_t h);
size_t ezkl_hip_bases_len(ezkl_bases_t h);
/* synthetic base set for benchmarks/tests (no public SRS without network, src/pfsys/srs.rs:10-11):
 * n deterministic curve points by try-and-increment, generated on the device */
int ezkl_hip_bases_generate(uint64_t seed, size_t first, size_t n, ezkl_bases_t* out_handle);
int ezkl_hip_bases_download(ezkl_bases_t h, void* out_host /* n x 64 B */);
/* Is every record in [first, first + n) of a resident set a point of G1?  The verdict of halo2's RawBytes reader (Params::read behind
 * load_srs_prover, src/pfsys/srs.rs:30-47 of the reference), per 64-byte record: reason 1 = x >= q, 2 = y >= q, 3 = y^2 != x^3 + 3, the
 * first that applies; the all-zero record is the identity, valid and counted apart (csrc/srs_check.hpp holds the predicate).
 * out[0] = invalid points, out[1] = the smallest invalid index (in the set, not relative to first) or UINT64_MAX, out[2] = the reason of
 * that point, out[3] = identities.  first + n beyond the set: EZKL_ERR_INVALID; n = 0 writes {0, UINT64_MAX, 0, 0}.  Reads the records the
 * handle holds, never the window tables (and builds none); one kernel, 47 us for 2^20 points on an MI355X. */
int ezkl_hip_bases_check(ezkl_bases_t h, size_t first, size_t n, uint64_t out[4]);
/* base set bases[i] = scalars[i] * P for one point P (64 B affine, host) and n resident Montgomery scalars: SRS
 * generation for tests (gen_srs -> ParamsKZG::setup, /root/reference/src/pfsys/srs.rs:14-16): g[i] = s^i G,
 * g_lagrange[i] = L_i(s) G */
int ezkl_hip_bases_from_scalars(const void* base_point, const void* scalars_dev, size_t n, ezkl_bases_t* out_handle);
/* per-row product: a NEW resident set of n points, out[i] = scalars[i] * in[first + i], for n resident Montgomery scalars laid out as
 * ezkl_hip_bases_from_scalars takes them (n x 32 B).  The step of an SRS update, g'[i] = t^i g[i] (backend.update_srs).
 * Output records are canonical affine; the identity -- an identity input, a zero scalar -- is the all-zero record.  first + n beyond the
 * set: EZKL_ERR_INVALID.  n = 0: EZKL_ERR_INVALID as well, since a base-set handle cannot be empty (ezkl_hip_bases_upload refuses
 * n = 0 too).  Reads the records the handle holds, never the window tables (and builds none); `in` is unchanged and nothing is kept
 * across calls.  One kernel, one lane per point, the double-and-add of ezkl_hip_bases_from_scalars with the point in vector registers,
 * 43.6 ms for 2^20 points on an MI355X, level with that call at the same n;
 * HIP events around it: ezkl_hip_last_kernel_ms("bases_mul_scalars") (and "bases_from_scalars" for the call above). */
int ezkl_hip_bases_mul_scalars(ezkl_bases_t in, const void* scalars_dev, size_t first, size_t n, ezkl_bases_t* out_handle);
/* ParamsKZG::downsize(new_k) -- halo2; called by load_params_prover (/root/reference/src/execute.rs:1739-1750) whenever the SRS file is
 * larger than the circuit, the normal case with a shared kzg22.srs: `g` (at least 2^new_k points of the coefficient basis s^i G) ->
 * out_g = its first 2^new_k points (may be NULL), out_g_lagrange = the Lagrange basis of the 2^new_k-point domain, L_i(s) G, computed as
 * halo2's g_to_lagrange does: an inverse NTT over G1 (omega^-1 butterflies on group elements, scaled by 1 / 2^new_k).  New handles,
 * freed with ezkl_hip_bases_free. */
int ezkl_hip_bases_downsize(ezkl_bases_t g, uint32_t new_k, ezkl_bases_t* out_g, ezkl_bases_t* out_g_lagrange);
/* sum_i scalars[i] * points[i] over G2 (the twist over Fq2).  points: n x 128 B affine -- x.c0, x.c1, y.c0, y.c1 as 32-byte little-endian
 * Montgomery Fq, the layout of the g2 / s_g2 tail of an SRS file, (0, 0) = identity; scalars: n x 32 B Montgomery Fr; out: 128 B canonical
 * affine.  Host pointers, borrowed.  On the reference's prove path G2 is data (the verifier's pairing consumes g2 and s_g2); the one G2
 * computation is gen_srs's s_g2 = [s] g2 (/root/reference/src/pfsys/srs.rs:14-16 -> ParamsKZG::setup), i.e. n = 1.  A plain
 * double-and-add per pair with a tree fold: not a Pippenger pipeline, not a hot path. */
int ezkl_hip_msm_g2(const void* points_affine, const void* scalars, size_t n, void* out_affine);
/* sum_i scalars[i] * bases[offset + i], i < n.  scalars: n x 32 B Montgomery Fr (host pointer, borrowed).
 * out_affine: 64 B, caller-allocated, canonical affine ((0,0) if the sum is the identity). */
int ezkl_hip_msm_g1(ezkl_bases_t h, const void* scalars, size_t n, void* out_affine);
/* same with scalars already resident in HBM; `stream` is a hipStream_t or NULL (library stream).
 * The result is written to host memory and the call returns after the stream has drained. */
int ezkl_hip_msm_g1_dev(ezkl_bases_t h, size_t base_offset, const void* scalars_dev, size_t n,
                        void* out_affine, void* stream);
/* sum_i scalars[i] * bases[base_offset + i] WITHOUT window tables: none is read, none is built, none is kept -- for a base set that is
 * uploaded, used for a few MSMs and freed (an SRS under check, a one-shot commit), where the ~55 ms table build of 2^20 points would
 * outweigh the MSMs.  Every window of the signed-digit recoding is summed by the chain of the fixed-base path over the raw records (W
 * window sums as fused groups of one sequence of launches, combined on the host: msm.hip, msm_once_run; DESIGN.md §4.1 "MSM without
 * window tables" has the cost and the measured times).  Results and errors as ezkl_hip_msm_g1_dev: canonical affine, (0,0) for the
 * identity, returns after the stream has drained; n = 0 and a range that runs past the set are EZKL_ERR_INVALID.  A handle that HAS a
 * table may be used here as well: the table is ignored.  Scratch is kept between calls (grown on demand, no allocation in steady state).
 * HIP events around the device work: ezkl_hip_last_kernel_ms("msm_once").  Not for a proving session: on prepared tables an MSM of 2^20
 * points takes 1.2 ms where this call takes 2.2 (0.6 against 1.5 on witness-like scalars). */
int ezkl_hip_msm_g1_once_dev(ezkl_bases_t h, size_t base_offset, const void* scalars_dev, size_t n, void* out_affine, void* stream);
/* the same over n points that are no base set: points_dev = n x 64 B affine Montgomery records, (0,0) = identity, resident (16-byte
 * aligned; read, never written) -- a verifier's commitments, a random combination of proof points */
int ezkl_hip_msm_g1_points_dev(const void* points_dev, const void* scalars_dev, size_t n, void* out_affine, void* stream);
/* 1 if the handle has a window table (built or being built: a fixed-base MSM or ezkl_hip_bases_prepare has run on it), else 0 */
int ezkl_hip_bases_has_table(ezkl_bases_t h);
/* batch of `batch` scalar vectors against the same bases (one commit per advice column) */
int ezkl_hip_msm_g1_batch(ezkl_bases_t h, const void* const* scalars, size_t batch, size_t n, void* out_affine);
/* One MSM in two halves: start queues it behind what the library stream has been asked to do so far (the scalar column may still be in
 * the making there) and returns a token; finish waits and writes the 64-byte affine point.  In between the caller may issue any other
 * call of this header -- commit batches and upload phases included: the MSM runs on a call slot with its own stream and scratch.  At most
 * four may be in flight per context: a fifth start WAITS while other threads hold the slots, and returns EZKL_ERR_BUSY when the calling
 * thread itself holds all four (it could never finish one).  finish takes a token exactly once, from any thread; a token that is not in
 * flight (never started, already finished, being finished by another thread) is EZKL_ERR_INVALID.  (The prover commits the vanishing argument's random polynomial, which depends on nothing but the
 * randomness, under the upload of the witness: halo2 draws it at the same place of the RNG stream either way.) */
int ezkl_hip_msm_g1_start_dev(ezkl_bases_t h, size_t base_offset, const void* scalars_dev, size_t n, int* token);
int ezkl_hip_msm_g1_finish(int token, void* out_affine);
/* the same with every scalar vector resident in HBM (array of DEVICE pointers held in host memory); the MSMs are
 * pipelined over several streams so the short reduce/sort kernels of one overlap the accumulation of the next */
int ezkl_hip_msm_g1_batch_dev(ezkl_bases_t h, size_t base_offset, const void* const* scalars_dev, size_t batch, size_t n,
                              void* out_affine, void* stream);
/* the same for WITNESS-SHAPED columns -- the caller knows that most scalars are small (advice columns, lookup multiplicities: one or
 * two non-zero window digits each).  Such an MSM is a chain of ~17 latency-bound launches whatever its length, so the batch runs as
 * fused groups of four columns per chain.  Any scalars are accepted (the result is the same); uniform ones just run a little slower. */
int ezkl_hip_msm_g1_batch_small_dev(ezkl_bases_t h, size_t base_offset, const void* const* scalars_dev, size_t batch, size_t n,
                                    void* out_affine, void* stream);
/* the same pipeline fed one column at a time, for callers that PRODUCE columns one by one on the device (compressed
 * lookup columns, grand products): the MSM of column j runs while column j+1 is being computed.  (It does not help for
 * columns arriving through blocking copies from pageable host memory: those queue behind the kernels in flight --
 * measured 36 vs 22 ms for 14 columns at k = 20 -- so the prover uploads first and commits in one batch.)  push returns
 * once the column's kernels are queued (it may first retire the oldest in-flight MSM); finish drains, writes `pushed`
 * affine points (EZKL_ERR_INVALID if capacity is smaller) and closes the batch, also on error.  One batch may be open at a
 * time; the other MSM entry points return EZKL_ERR_INVALID while it is. */
/* One prover phase in one call (create_proof: "assign advice, blind, commit"): host_cols[j] (n x 32 B) is copied into the
 * caller's device column dev_cols[j], rows [tail_start, tail_start + tail_count) are overwritten with tail_rows[j] (the blinding
 * values; tail_rows may be NULL) and rows [commit_first, commit_first + commit_count) of the column are committed against
 * bases [0, commit_count) (the whole column: 0, n; a rank holding one slice of the SRS: its slice); out_affine gets `batch` points.
 * Every copy is queued at once on a dedicated copy stream and the MSM of column j only waits for ITS copy, so the PCIe
 * traffic of the later columns runs under the kernels of the earlier ones.  Page-locked host columns
 * (ezkl_hip_host_malloc) make the copies asynchronous; pageable ones work but are staged by the runtime. */
int ezkl_hip_upload_commit_batch(ezkl_bases_t h, const void* const* host_cols, void* const* dev_cols, size_t batch, size_t n,
                                 const void* const* tail_rows, size_t tail_start, size_t tail_count, size_t commit_first, size_t commit_count,
                                 void* out_affine);
/* The same phase in steps, for callers that want other work to start as each column lands (the prover queues the iNTT and the
 * coset NTT of an advice column on its own stream while later columns are still crossing PCIe and earlier ones are being
 * committed): begin queues every copy and returns at once (the host columns must stay valid until end); wait makes `stream` (a
 * caller stream, not NULL) wait for column j; commit runs the MSMs (each waits for its own column) and returns the `batch`
 * points; end drains the copy stream and closes the phase, also after an error.  One phase may be open at a time. */
typedef struct ezkl_upload_s* ezkl_upload_t;
int ezkl_hip_upload_begin(const void* const* host_cols, void* const* dev_cols, size_t batch, size_t n, const void* const* tail_rows,
                          size_t tail_start, size_t tail_count, ezkl_upload_t* out_upload);
/* begin with a FORMAT per host column: what crosses PCIe need not be 32 bytes per cell.  Every cell of an ezkl advice column is
 * integer_rep_to_felt of an IntegerRep (i128: the quantised tensor value; /root/reference/src/fieldutils.rs:6-17) before halo2 sees it as an
 * Fp, so a caller that still has the integers hands THOSE over -- 16 bytes per cell, or 8 when every value of the column fits an int64
 * -- and the column is expanded on the device (x >= 0 -> x, x < 0 -> r - |x|, then the Montgomery form) as its copy lands; the device
 * column, the blinding rows (tail_rows: always 32-byte Montgomery words) and the commitment are bit for bit those of the 32-byte form.
 * formats == NULL: every column EZKL_COLUMN_FP (= ezkl_hip_upload_begin). */
#define EZKL_COLUMN_FP 0        /* 32-byte Montgomery words, halo2curves' in-memory Fr */
#define EZKL_COLUMN_INT64 1     /* int64_t per cell */
#define EZKL_COLUMN_INT128 2    /* little-endian two's-complement 128-bit integer per cell (Rust's i128 = ezkl's IntegerRep) */
/* the "host" pointer is a DEVICE column of 2^k 32-byte Montgomery words (ezkl_hip_malloc; e.g. filled by ezkl_hip_witness_run_dev): it is
 * copied into the destination column on the device -- no host round trip -- and left unmodified (the blinding rows go into the copy).
 * Everything queued on the library stream has run before the copy starts; a column written on another stream must be complete. */
#define EZKL_COLUMN_DEVICE_FP 3
int ezkl_hip_upload_begin_fmt(const void* const* host_cols, const uint8_t* formats, void* const* dev_cols, size_t batch, size_t n,
                              const void* const* tail_rows, size_t tail_start, size_t tail_count, ezkl_upload_t* out_upload);
int ezkl_hip_upload_wait(ezkl_upload_t upload, size_t column, void* stream);
int ezkl_hip_upload_commit(ezkl_upload_t upload, ezkl_bases_t h, size_t commit_first, size_t commit_count, void* out_affine);
int ezkl_hip_upload_end(ezkl_upload_t upload);
/* ---- witness synthesis on the device from a recorded plan: replaces the per-cell host pass of GraphCircuit::synthesize
 *      (/root/reference/src/graph/mod.rs:2010-2200) for the op family whose cell positions do not depend on the input -- the MLP ops of
 *      /root/reference/src/circuit/ops/layouts.rs: dot :532-610, pairwise :2917-2990, equals_zero :3549-3580, enforce_equality :4959-4981,
 *      range_check :5024-5105, decompose :6321-6423, leaky_relu at slope 0 :6457-6474, output :6740-6779 -- and static lookups
 *      (nonlinearity :5143-5222), which with those ops is the conv2d_mnist example's layout ----
 * A PLAN is the layout recorded once per circuit (ezkl_amd/witness_plan.py; byte layout: csrc/witness_plan.hpp): a list of records, each a
 * batch of cell writes of one kind (copy, const, input, param, add / sub / mult, decompose hint, range-check index, inverse-or-zero, dot,
 * static-lookup output, static-lookup table-column index, integer matmul, random linear combination, rounded division by a constant, running sum, running product, gather, clamp, sort, argsort,
 * claimed reciprocal, claimed square root, claimed arg-extremum, claimed scatter, claimed complement, claimed one-hot vector) with u32 cell indices column * 2^k + row, a table of int64 parameters, a table
 * of constants and -- header words 12 / 13 (n_tables, n_table_values; zero, as reserved words were, in a plan without lookups), after the
 * pool -- a directory of {lo (int32), n, col_size, offset} per static lookup table and the tables' values f(lo + i) as int64.  The version
 * word stays 1.  A lookup record names its source cells and a table: with s the signed value of the cell, the output kind writes
 * values[offset + (s - lo)] as a field element (negative: r - |v|), the index kind (s - lo) // col_size.
 * upload: the blob is validated on the HOST first -- version, every cell index < n_advice * 2^k, every table index in range, every lookup
 *   table inside the values with n >= 1, col_size >= 1 and lo + n - 1 <= 2^31 - 1, every cell written once and read only after an earlier
 *   record wrote it -- and refused with EZKL_ERR_INVALID otherwise (also without a device;
 *   ezkl_hip_witness_last_error says why); then its tables go to the device, where they are read-only.  n_advice <= 64.
 * run: zero-fills the n_advice columns (device, 2^k x 32 bytes each, distinct, e.g. from ezkl_hip_malloc), uploads the n_inputs int64
 *   model inputs (they enter the field as EZKL_COLUMN_INT64 cells do) and replays the plan, ONE launch per record, on `stream` (NULL: the
 *   library stream); returns after the stream has drained with outputs_host = the circuit's outputs (32-byte Montgomery words) and
 *   status = {cells that failed, (record << 32 | element) of the first, cells written, launches (fills included)}.  A value that does
 *   not fit its decomposition (|x| >= base^legs, the layout's "value exceeds the decomposition range") is counted by the kernel -- nothing
 *   traps, the process goes on -- and the call returns EZKL_ERR_INVALID with ezkl_hip_witness_last_error naming the op, record and
 *   element; the columns are then not a witness.  A lookup input outside its table (s < lo, s > lo + n - 1, |s| >= 2^62: the layout's
 *   "lookup input outside the table range") is reported the same way, with that message.  So is the dividend of a division record (kind 15:
 *   a = source cell, p0 = d >= 1, a zero divisor is refused on upload; with s the signed value of the cell it writes sgn(s) * ((|s| + d / 2) / d),
 *   the rounded quotient layouts.rs:219-267 `div` claims) with |s| >= 2^52: "rebase dividend outside the exact-division range".  Scratch belongs to the plan (column pool): nothing is allocated per run, and a plan
 *   runs one synthesis at a time.  HIP events around the run: ezkl_hip_last_kernel_ms("witness").
 * info: out = {k, n_advice, n_inputs, n_outputs, n_records, n_cells, n_ops (layout-op calls recorded), n_params}.
 * PHASES (second-phase advice: the Freivalds einsum, /root/reference/src/circuit/ops/chip/einsum/mod.rs:96-309).  Header word 14 of the blob is
 *   n_challenges, word 15 n_phases (0 reads as 1), the eighth word of a record its phase -- all three were reserved zeros, so every one-phase
 *   blob keeps its bytes and the version word stays 1.  Phases are non-decreasing along the record list; a column belongs to the phase of the
 *   records that write it (never to two; a column no record writes: phase 0); input and matmul records belong to phase 0.  Two record kinds
 *   serve the einsum: matmul -- count = m * n, p0 = kd, p1 = n, a / b = m * kd / kd * n input indices: dst[i * n + j] = sum_t in[a[i * kd + t]] *
 *   in[b[t * n + j]] over the integers, then integer_rep_to_felt; every operand must satisfy |v| < 2^31, one outside is reported as a value
 *   beyond its decomposition is ("einsum operand outside the exact-product range", element = its place in a, or m * kd + its place in b) --
 *   and rlc -- count scans of p1 steps with challenge p0, step-major and dense: out[0] = c * v[0], out[t] = out[t - 1] * c + c * v[t].
 * run_phase: one phase of a plan, between the prover's commit stages.  challenges = n_challenges x 32 bytes, little-endian CANONICAL scalars
 *   (the ones squeezed so far; a non-canonical one: EZKL_ERR_INVALID).  The run zero-fills and writes the columns of ITS phase only; the
 *   inputs are taken with phase 0 (later phases ignore inputs_host / n_inputs), the outputs are gathered by the last phase (outputs_host may
 *   be NULL before).  Phase p > 0 needs a phase p - 1 that ran to its end on the same column pointers since the last phase 0 -- it reads
 *   those cells where they are -- and is refused otherwise (EZKL_ERR_INVALID, "phase 1 before phase 0 ...", nothing is launched).  status as
 *   for run, per phase.  ezkl_hip_witness_run_dev on a one-phase plan is run_phase(0); on a plan with phases it returns EZKL_ERR_INVALID and
 *   names this call.
 * phases: out = {n_phases, n_challenges}; column_phase (may be NULL): n_advice bytes, the phase each column belongs to.
 * THE SURROGATE'S OPS (kinds 17 - 20, appended; kind 16 stays unassigned and is refused as unknown; the version word stays 1 and every earlier
 *   blob keeps its bytes).  sum / prod (17 / 18:
 *   BaseRegion._accumulate, layouts.rs:2472-2621) -- count scans of p1 steps with p0 operands each, step-major as dot is: step s of scan d folds
 *   the cells a[(s * p0 + j) * count + d], j < p0 (0xffffffff: no operand), into the running value (0 for a sum, 1 for a product) and writes it to
 *   dst[s * count + d] (0xffffffff: no such step); b is unused.  gather (19) -- element-wise: a = the cell holding the index, p0 = the pool offset
 *   of the table's cell list, p1 = its length n >= 1; with s the signed value of the index cell the destination gets the value of cell
 *   pool[p0 + s]; every listed cell must have been written by an earlier record.  s < 0, s >= n or |s| >= 2^62 is reported as a value beyond
 *   its decomposition is ("gather index outside the table"); the lane tests s before it reads pool[p0 + s].  clamp (20) -- element-wise:
 *   a = source cell, p0 = lo, p1 = hi (int32, lo <= hi): min(max(s, lo), hi); a value beyond 62 bits clamps by its sign; it never fails.
 * SORT AND TOP-K (kinds 21 / 22, appended; the version word stays 1 and every earlier blob keeps its bytes): the witness of layouts.rs:1158-1275
 *   `_sort_ascending` -- the sorted tensor and the claimed indices of its permutation argument.  sort (21) / argsort (22): count destination
 *   cells dst[e] in segments of p0 = n elements (n >= 1, count % n == 0, count <= 2^28), p1 = mode (0: the position ascending among equal values,
 *   1: descending), a = the source cells, segment-major and dense, b unused; anything else is refused on upload ("bad sort shape").  The order of a
 *   segment is by (signed value, position), a total order.  sort: dst[s * n + i] gets the i-th smallest signed value of the cells a[s * n .. + n)
 *   as a field element (negative: r - |v|); argsort: the position, in [0, n), of that element in its segment.  A source with |s| >= 2^62 is
 *   reported as a value beyond its decomposition is ("sort key beyond 62 bits", element = its place in a, once per record that reads it) and
 *   its SEGMENT writes none of its cells; the other segments of the record are written.  Segments of up to 2048 elements (padded to a power of
 *   two) are sorted in ONE launch, 2048 keys to a workgroup; a longer one takes several launches on the stream through key scratch the plan owns
 *   (the largest record's segments x padded length x 16 bytes, from the column pool at upload): `launches` counts them all.
 * RECIPROCAL AND SQUARE ROOT (kinds 24 / 25; kind 23 stays unassigned as 16 does, the version word stays 1 and every earlier blob keeps its
 *   bytes): the claims of layouts.rs:300-385 `recip` and :408-459 `sqrt`, in exact integers.  recip (24) -- element-wise: a = source cell,
 *   b = the index of `zero_inverse` in the constants section (one word, not a pool offset), p0 / p1 = the low / high word of S = input scale *
 *   output scale, 1 <= S < 2^62.  With x the signed value of the cell: x = 0 -> that constant; x > 0 -> ceil((2S - x) / (2x)); x < 0 ->
 *   -floor((2S + |x|) / (2|x|)): the smallest integer minimiser of |y * x - S|, the one value the gates of `optimum_convex_function` accept
 *   (the f64 formula of the reference differs from it at exact ties with x > 0, where the reference's own gates refuse the f64 value).
 *   |x| >= 2^62 is reported as a value beyond its decomposition is ("reciprocal operand beyond 62 bits").  sqrt (25) -- element-wise: a =
 *   source cell, b = 0, p0 = input scale >= 1, p1 = 0.  With T = x * p0: T <= 0 -> 0; else r = floor(sqrt(T)), r + (T - r * r > r), the
 *   integer nearest to sqrt(T).  |x| >= 2^62 or T >= 2^62 is reported likewise ("square-root operand outside the exact range").  S = 0,
 *   S >= 2^62, a constant index past the constants, a zero scale or p1 != 0 on sqrt are refused on upload.
 * ARGMAX AND ARGMIN (kind 27; kind 26 stays unassigned as 16 and 23 do, the version word stays 1 and every earlier blob keeps its bytes): the
 *   index layouts.rs:5225-5293 `argmax` / `argmin` claim before the sort that checks it.  argext (27): count segments of p0 = n >= 1 source
 *   cells and as many destination cells dst[s], p1 = mode (0: argmax, 1: argmin), a = the count * n source cells, segment-major and dense, b
 *   unused; n = 0, a mode above 1, count * n > 2^28 or an array past the pool is refused on upload ("bad arg-extremum shape").  dst[s] gets the
 *   SMALLEST position in [0, n) whose signed value is the greatest (least) of the cells a[s * n .. + n): max_by_key((value, -idx)) /
 *   min_by_key((value, idx)) of the reference, the one claim its gates accept.  A source with |s| >= 2^62 is reported as a value beyond its
 *   decomposition is ("arg-extremum key beyond 62 bits", element = its place in a) and its segment's cell is not written; the other segments
 *   of the record are.  Segments of up to 64 sources are reduced side by side in a wave, up to 4096 by one workgroup each, in ONE launch; a
 *   longer one takes two launches through the key scratch the plan owns (shared with the sort kinds, sized at upload to the larger need):
 *   `launches` counts them all.
 * GATHER, SCATTER AND ONE-HOT (kinds 29 - 31; kind 28 stays unassigned as 16, 23 and 26 do, the version word stays 1 and every earlier blob keeps
 *   its bytes): the three claims of the indexed family that depend on the data.  scatter (29) -- ONE tensor, the claimed output of
 *   layouts.rs:2313-2379 `scatter_elements`: count = n destination cells dst[i], a = the n base cells, p0 = m >= 1 elements, p1 = the multiplier
 *   of the scattered dimension >= 1, b = the pool offset of 1 + 3m words: the extent of that dimension, m index cells, m source cells, m
 *   constant offsets (plain words).  With s_j the signed value of index cell j its target is t_j = s_j * p1 + off_j; dst[i] gets the value of
 *   source cell j for the GREATEST j with t_j == i (the later element wins), else the value of base cell i.  p0, p1 or the extent zero, count >
 *   2^28, an array past the pool or an offset with off_j + (extent - 1) * p1 >= count is refused on upload ("bad scatter shape").  s_j < 0,
 *   s_j >= extent or |s_j| >= 2^62 is reported as a value beyond its decomposition is ("scatter index outside the tensor", element = j, every
 *   such j counted) and the record writes none of its cells.  complement (30) -- the claimed output of layouts.rs:2213-2286
 *   `get_missing_set_elements` over the positions: p0 = n, p1 = m <= n source cells at a, count = n - m destination cells (zero is legal: no
 *   cell, no launch), b unused; dst[i] gets the i-th smallest v in [0, n) that is the signed value of no source cell; a source outside [0, n)
 *   or beyond 62 bits removes nothing; it never fails.  p1 > p0, count != p0 - p1, p0 > 2^28 or an array past the pool is refused on upload
 *   ("bad complement shape").  one_hot (31) -- element-wise, the claimed vector of layouts.rs:1398-1442 `one_hot`: a = the index cell of the
 *   element, b = the pool offset of the per-element positions (plain words), p0 = the number of classes >= 1 ("zero one-hot classes"), p1 = 0:
 *   1 if the signed value equals the position, else 0.  s < 0, s >= p0 or |s| >= 2^62 is reported likewise ("one-hot index outside the
 *   classes") and the lane writes nothing.  A scatter or a complement of up to 4096 cells runs in ONE launch, one workgroup with its winner
 *   words or presence flags in LDS; a longer one takes three (fill, mark, store) or up to five (fill, mark, count, offsets, compact) launches
 *   through the scratch the plan owns (shared with the sort and arg-extremum kinds, sized at upload to the largest need): `launches` counts them all.
 * tile: a plan of a tiled circuit writes rows [0, U) of the block-0 and shared columns; the circuit is those U rows repeated T times down every
 *   column and copied into the columns of the other blocks.  For every pair, rows [t * U, (t + 1) * U) of column dst get rows [0, U) of column
 *   src: t = 0 .. T - 1 when dst != src, t = 1 .. T - 1 when dst == src.  Rows >= T * U and columns outside the pair list are left as they are.
 *   One launch on `stream` (NULL: the library stream), not waited for; HIP events around it: ezkl_hip_last_kernel_ms("witness_tile").  Nothing
 *   is launched and the call returns EZKL_ERR_INVALID when U = 0 or T = 0, U * T > 2^k, a column index >= n_advice (<= 64), a column appears twice
 *   as dst, a column that is some pair's src is another pair's dst with dst != src (its rows [0, U) would be written while they are read), or
 *   two of the columns named share a buffer.
 * lookup_stats: the statistics a witness file carries of a circuit with static lookups (GraphWitness min_lookup_inputs / max_lookup_inputs,
 *   which the reference's layout keeps in region.rs:548-559): over the source cells of every nonlinearity (11) record of the plan, in all
 *   phases, the least and the greatest signed value, both folded with 0 -- a plan without such a record answers (0, 0) and launches
 *   nothing.  advice_cols_dev: the n_advice columns of a run that returned EZKL_OK (every source is then canonical and inside its table; the
 *   columns of a refused run are not to be passed).  A source whose magnitude needs 62 bits or more makes the call return EZKL_ERR_INVALID
 *   (ezkl_hip_witness_last_error counts them) with out_min_max = (0, 0) rather than a wrong extremum.  One launch: a lane per element,
 *   striding over the records; one 64-bit atomicMin and one atomicMax per wave on two result words the plan owns, set to 0 by every call.
 *   The call waits for its result; HIP events around the launch: ezkl_hip_last_kernel_ms("witness_lookup_stats").
 * outputs: the plan's output cells before its last phase -- run_phase gathers them with the LAST phase only, and the instance column is
 *   needed before the first commitment.  advice_cols_dev: the n_advice column pointers phase 0 last ran to its end on; outputs_host
 *   receives n_outputs x 32 bytes, Montgomery words, as run's does.  One gather launch, one copy, one wait; HIP events around the launch:
 *   ezkl_hip_last_kernel_ms("witness_outputs").  Before phase 0 has succeeded, on other column pointers than it ran on, or with an
 *   output cell in a column of a phase that has not run to its end, the call returns EZKL_ERR_INVALID, ezkl_hip_witness_last_error says
 *   which, and nothing is launched.  A plan without outputs: EZKL_OK, nothing launched. */
typedef struct ezkl_wplan_s* ezkl_wplan_t;
typedef ezkl_wplan_t ezkl_witness_plan_t;
int ezkl_hip_witness_plan_upload(const void* blob, size_t len, ezkl_wplan_t* out_plan);
int ezkl_hip_witness_plan_free(ezkl_wplan_t plan);
int ezkl_hip_witness_plan_info(ezkl_wplan_t plan, uint32_t out[8]);
int ezkl_hip_witness_run_dev(ezkl_wplan_t plan, const int64_t* inputs_host, size_t n_inputs, void* const* advice_cols_dev, void* outputs_host,
                             uint64_t status[4], void* stream);
int ezkl_hip_witness_run_phase_dev(ezkl_wplan_t plan, uint32_t phase, const int64_t* inputs_host, size_t n_inputs, const void* challenges, size_t n_challenges,
                                   void* const* advice_cols_dev, void* outputs_host, uint64_t status[4], void* stream);
int ezkl_hip_witness_plan_phases(ezkl_wplan_t plan, uint32_t out[2], uint8_t* column_phase);
int ezkl_hip_witness_tile_dev(void* const* advice_cols_dev, uint32_t n_advice, uint32_t k, uint32_t unit_rows, uint32_t tiles, const uint32_t* dst_cols,
                              const uint32_t* src_cols, uint32_t n_pairs, void* stream);
int ezkl_hip_witness_lookup_stats_dev(ezkl_witness_plan_t plan, void* const* advice_cols_dev, int64_t out_min_max[2], void* stream);
int ezkl_hip_witness_outputs_dev(ezkl_witness_plan_t plan, void* const* advice_cols_dev, void* outputs_host, void* stream);
const char* ezkl_hip_witness_last_error(void);   /* the calling thread's last refusal (upload) or range failure (run); "" after a success */
/* Which kernel replayed the DOT records: *launches = how many of them, in this process so far, went to the wide kernel -- a record of ONE step
 * (p1 == 1) with p0 >= 16 products, the claimed product of an einsum, every lane of a wave multiplying -- instead of the chunked scan every
 * other DOT record runs on.  reset != 0 sets the count back to zero after reading it.  The cells do not depend on the kernel. */
int ezkl_hip_witness_wide_dots(uint64_t* launches, int reset);
/* A commit batch fed as its columns become final: begin; push (one column / several: fused into groups as the one-call batch does) any
 * number of times; finish returns the points in push order and closes the batch (also after an error).  A push returns once the MSMs
 * are QUEUED: they start behind everything queued on the library stream so far (an event, no host synchronisation), on the MSM slot
 * streams, so the caller can go on queuing unrelated library-stream work while they run -- the prover commits the permutation
 * products z while the lookup arguments' running sums are still being computed.  The pushed columns must stay untouched until finish.
 * One batch may be open per context; the other MSM entry points refuse (EZKL_ERR_INVALID) until it is finished. */
typedef struct ezkl_msm_batch_s* ezkl_msm_batch_t;
int ezkl_hip_msm_batch_begin(ezkl_bases_t h, size_t base_offset, size_t n, ezkl_msm_batch_t* out_batch);
int ezkl_hip_msm_batch_push_dev(ezkl_msm_batch_t batch, const void* scalars_dev);
int ezkl_hip_msm_batch_push_many_dev(ezkl_msm_batch_t batch, const void* const* scalars_dev, size_t count);
int ezkl_hip_msm_batch_finish(ezkl_msm_batch_t batch, void* out_affine, size_t capacity);
/* out = a + b on affine points (host, used to fold per-GPU partial sums after the all-gather) */
int ezkl_hip_g1_add_affine(const void* a, const void* b, void* out);

/* ---- NTT: replaces halo2curves::fft::best_fft / EvaluationDomain::{ifft, coeff_to_extended,
 *      extended_to_coeff} (type used in-tree at /root/reference/src/circuit/modules/polycommit.rs:52) ---- */
/* best_fft(data, omega, log_n): natural order in and out; if `inverse`, additionally scales by 1/n
 * (omega is then the inverse root, as EvaluationDomain::ifft passes it).  Host buffer, in place. */
int ezkl_hip_ntt(void* data, uint32_t log_n, const void* omega, int inverse);
/* device-resident batch: `batch` columns of 2^log_n elements, column b at data_dev + b*stride_elems*32 */
int ezkl_hip_ntt_dev(void* data_dev, uint32_t log_n, const void* omega, int inverse,
                     size_t batch, size_t stride_elems, void* stream);
/* coeff_to_extended (inverse = 0): in[b] has 2^log_n coefficients, out[b] gets 2^log_n_ext evaluations on
 * the zeta-coset.  extended_to_coeff (inverse = 1): in[b] has 2^log_n_ext evaluations, out[b] receives
 * 2^log_n_ext coefficients (caller truncates).  Host pointers.  in == out allowed when sizes match. */
int ezkl_hip_coset_ntt_batch(const void* const* in, void* const* out, size_t batch,
                             uint32_t log_n, uint32_t log_n_ext, int inverse);
int ezkl_hip_coset_ntt_dev(const void* in_dev, void* out_dev, size_t batch, size_t in_stride_elems,
                           size_t out_stride_elems, uint32_t log_n, uint32_t log_n_ext, int inverse, void* stream);

/* coeff_to_extended with the result in COSET-MAJOR order: the extended domain {zeta w_ext^i} is the union of E = 2^(log_n_ext - log_n)
 * cosets c_b H (c_b = zeta w_ext^b, H = <omega>), natural index i = E j + b; out[b 2^log_n + j] = p(c_b omega^j).  Computed as E
 * transforms of 2^log_n points (the zero-padding stages of the 2^log_n_ext-point transform never run).  A rotation by r rows of the
 * 2^log_n domain is a shift by r inside a coset, so ezkl_hip_eval_h_dev run with k = ext_k = log_n on the b-th cosets of its columns IS
 * the quotient sweep of coset b (and a coset is the unit a multi-GPU prover hands to a rank).  in != out.
 * ezkl_hip_cosets_transpose_dev converts one extended column between the two orders (to_natural = 1: coset-major -> natural, the order
 * of halo2's pk.key `*_cosets` sections and of ezkl_hip_coset_ntt_dev). */
int ezkl_hip_coeff_to_cosets_dev(const void* in_dev, void* out_dev, size_t batch, size_t in_stride_elems, size_t out_stride_elems,
                                 uint32_t log_n, uint32_t log_n_ext, void* stream);
int ezkl_hip_cosets_transpose_dev(const void* in_dev, void* out_dev, uint32_t log_n, uint32_t log_n_ext, int to_natural, void* stream);
/* the same for a RANGE of cosets: out[(b - first_coset) 2^log_n + j] = p(c_b omega^j) for b in [first_coset, first_coset + n_cosets),
 * n_cosets a power of two (out_stride_elems >= n_cosets 2^log_n).  A rank of a sharded prover sweeps only some cosets of the extended
 * domain and needs only those cosets of the key columns (fixed, sigma, l0 / l_last / l_active): 1 / world of the bytes and of the work. */
int ezkl_hip_coeff_to_cosets_range_dev(const void* in_dev, void* out_dev, size_t batch, size_t in_stride_elems, size_t out_stride_elems,
                                       uint32_t log_n, uint32_t log_n_ext, uint32_t first_coset, uint32_t n_cosets, void* stream);

/* ---- element-wise Fr vector ops (icicle vec-ops surface) on device-resident data ---- */
#define EZKL_VEC_ADD 0
#define EZKL_VEC_SUB 1
#define EZKL_VEC_MUL 2
int ezkl_hip_vec_op_dev(int op, const void* a_dev, const void* b_dev, void* out_dev, size_t n, void* stream);
int ezkl_hip_vec_scale_dev(const void* a_dev, const void* scalar_host, void* out_dev, size_t n, void* stream);
int ezkl_hip_vec_fill_dev(void* out_dev, const void* value_host, size_t n, void* stream);   /* out[i] = value */
/* One sigma column of the permutation argument (halo2 permutation::keygen::Assembly::build_pk: sigma_c[r] = delta^c' omega^r' where
 * (c', r') is the cycle successor of cell (c, r)): cells are numbered column position * 2^log_n + row; next_dev = the successors of the
 * 2^log_n cells of this column (u32, device), omega_col_dev[r] = omega^r, delta_pows_dev[c] = delta^c (n_columns entries).
 * out_dev[r] = delta_pows[t >> log_n] * omega_col[t mod 2^log_n], t = next_dev[r] (zero for a successor outside the n_columns). */
int ezkl_hip_permutation_sigma_dev(const void* next_dev, const void* omega_col_dev, const void* delta_pows_dev, uint32_t n_columns, uint32_t log_n,
                                   void* out_dev, void* stream);
/* a[i] *= t[i mod 2^(ext_k-k)], t = 1/((zeta*omega_ext^j)^n - 1): EvaluationDomain::divide_by_vanishing_poly */
int ezkl_hip_divide_by_vanishing_dev(void* a_dev, uint32_t k, uint32_t ext_k, void* stream);
/* running sum (EZKL_VEC_ADD) / running product (EZKL_VEC_MUL): out[i] = in[0] o ... o in[i] (inclusive) or
 * o in[i-1] with out[0] = identity (exclusive): the grand sum of mv-lookup::commit_grand_sum and the grand
 * product z(X) of permutation::commit.  in == out allowed. */
int ezkl_hip_prefix_scan_dev(int op, int exclusive, const void* in_dev, void* out_dev, size_t n, void* stream);
/* mv-lookup multiplicities m(X) (mv_lookup::prover::prepare): for every usable row r of every (theta-compressed) input
 * column, the FIRST usable table row holding the same value gets +1; m_out is an n_rows Fr column (rows >= usable
 * are 0).  *out_missing (may be NULL) = number of input values absent from the table (a failing witness). */
int ezkl_hip_lookup_multiplicity_dev(const void* const* inputs_dev, uint32_t n_inputs, const void* table_dev, uint32_t n_rows,
                                     uint32_t usable_rows, void* m_out_dev, uint32_t* out_missing, void* stream);
/* the same with the count of absent input values ADDED to a device u32 (missing_dev, zeroed by the caller): nothing returns to the
 * host, so the call is stream-ordered like the other helpers; a prover queues all its lookup arguments and reads the counter once */
int ezkl_hip_lookup_multiplicity_acc_dev(const void* const* inputs_dev, uint32_t n_inputs, const void* table_dev, uint32_t n_rows,
                                         uint32_t usable_rows, void* m_out_dev, void* missing_dev, void* stream);
/* every lookup argument of a proof in ONE call (mv_lookup::prover::prepare runs once per argument, on independent data): argument l has
 * the table tables_dev[l] and the output column m_outs_dev[l]; input column j (n_inputs of them in all, any number per argument)
 * belongs to argument input_lookup[j].  Three launches for the whole batch instead of three per argument -- the passes are random
 * 4- and 32-byte reads, and one argument alone leaves most of the machine waiting on them.  missing_dev as in _acc_dev. */
int ezkl_hip_lookup_multiplicity_batch_dev(const void* const* inputs_dev, const uint32_t* input_lookup, uint32_t n_inputs, const void* const* tables_dev,
                                           uint32_t n_lookups, uint32_t n_rows, uint32_t usable_rows, void* const* m_outs_dev, void* missing_dev, void* stream);
/* halo2 eval_polynomial(poly, x): sum_i coeffs[i] * x^i for a resident coefficient vector; x and the 32-byte result
 * are host memory (create_proof evaluates every queried (column, rotation) this way before SHPLONK) */
int ezkl_hip_eval_poly_dev(const void* coeffs_dev, size_t n, const void* x_host, void* out_host, void* stream);
/* m evaluations in one call: polynomial j (n coefficients, resident) at xs[j] (host, m x 32 B) -> out_host[j]; one upload,
 * one download, one synchronisation for the whole batch of create_proof's step 10 */
int ezkl_hip_eval_poly_batch_dev(const void* const* coeffs_dev, const void* xs_host, uint32_t m, size_t n, void* out_host, void* stream);
/* out[i] = (accumulate ? out[i] : 0) + sum_j coeffs[j] * inputs[j][i]: the linear combinations of SHPLONK
 * (ProverSHPLONK::create_proof) and the x^n-Horner over the quotient pieces, each input read once.  inputs: m DEVICE
 * pointers in host memory; coeffs: m x 32 B host */
/* q(X) = a(X) / (X - z), remainder dropped: out[n-1] = 0, out[i-1] = a[i] + z out[i] (halo2_proofs::arithmetic::kate_division,
 * the quotients of the KZG / SHPLONK openings).  n coefficients resident, z host (32 B Montgomery); out may alias a. */
int ezkl_hip_kate_division_dev(const void* a_dev, const void* z_host, void* out_dev, size_t n, void* stream);
int ezkl_hip_lincomb_dev(const void* const* inputs_dev, const void* coeffs_host, uint32_t m, void* out_dev, size_t n, int accumulate,
                         void* stream);
/* out[i] = uniform element of Fr, i < n, expanded from a 256-bit key with ChaCha20 (64-bit block counter, 64-bit stream
 * id): element (first + i) owns blocks 16(first+i) .. +15; its 32 candidates are the 8-word halves of those blocks with
 * the top two bits cleared; the first candidate < r is taken (rejection sampling => uniform on [0, r)).  Replaces the
 * host-side OsRng loop of halo2 (blinding rows; vanishing::Argument::commit's random polynomial, 2^k elements) by a
 * keystream expanded where the column lives; the caller provides the key (OS entropy, or a seed for det-prove,
 * /root/reference/src/pfsys/mod.rs:436-439). */
int ezkl_hip_chacha20_fr_dev(const void* key32, uint64_t stream_id, size_t first, void* out_dev, size_t n, void* stream);
/* Montgomery batch inversion (zeros stay zero), in place */
int ezkl_hip_batch_invert_dev(void* a_dev, size_t n, void* stream);

/* ---- quotient numerator: replaces plonk::evaluation::Evaluator::evaluate_h's row sweep
 *      (GraphEvaluator::evaluate; icicle "gate_eval" program on the GPU build) ---- */
/* instruction = 8 x u32: [op, target, s0.kind, s0.idx, s0.rot, s1.kind, s1.idx, s1.rot] (a unary op has s0 only).  An intermediate index
 * may be rewritten any number of times, also by an instruction that reads it; a HORNER_STEP on a target no instruction has written is
 * its term s0; a read of an intermediate that is not written at that point is EZKL_ERR_INVALID; the result is the last instruction's
 * target (tests/evalh_forms.py). */
enum { EZKL_OP_ADD = 0, EZKL_OP_SUB, EZKL_OP_MUL, EZKL_OP_SQUARE, EZKL_OP_DOUBLE, EZKL_OP_NEGATE,
       EZKL_OP_STORE, EZKL_OP_HORNER_STEP /* target = target*s1 + s0 */ };
enum { EZKL_SRC_CONST = 0, EZKL_SRC_INTERMEDIATE, EZKL_SRC_COLUMN, EZKL_SRC_CHALLENGE, EZKL_SRC_PREVIOUS };
typedef struct {
    const uint32_t* code;       uint32_t n_instr;  uint32_t n_intermediates;
    const void* constants;      uint32_t n_constants;     /* n x 32 B Fr, host */
    const int32_t* rotations;   uint32_t n_rotations;     /* in rows of the 2^k domain */
    const void* const* columns; uint32_t n_columns;       /* DEVICE pointers, each 2^ext_k x 32 B */
    const void* challenges;     uint32_t n_challenges;    /* n x 32 B Fr, host */
    uint32_t k, ext_k;
} ezkl_program_t;
/* Every word must be canonical (< r, Montgomery form): constants and challenges are checked (EZKL_ERR_INVALID otherwise); the column words
 * and out_dev are NOT -- every kernel of this library that produces a column writes canonical words, and a check of device columns would
 * cost a pass over them per call.  A non-canonical column word gives an undefined (possibly non-canonical) result for its rows. */
/* out_dev[r] = program(row r) with ValueSource::PreviousValue = old out_dev[r]; 2^ext_k rows.  The host arrays of `prog` are borrowed
 * for the call only (packed into pinned staging the library owns); on a caller stream, or on the library stream in asynchronous mode
 * (ezkl_hip_set_async), the call returns once the launch is queued -- the columns and out_dev must stay valid until it has run. */
int ezkl_hip_eval_h_dev(const ezkl_program_t* prog, void* out_dev, void* stream);
/* the sweep is JIT-compiled (hiprtc) into straight-line gfx950 code, once per program; this host-only call
 * checks that a program lowers and compiles (column pointers are not dereferenced; no GPU needed) */
int ezkl_hip_eval_h_check(const ezkl_program_t* prog);
/* host-only: the source ezkl_hip_eval_h_check would compile (the generator selected by EZKL_EVALH_R29; rotation offsets written as 0).
 * *len receives its length in bytes; it is copied NUL-terminated into out when cap > *len, else EZKL_ERR_INVALID (query with out = NULL) */
int ezkl_hip_eval_h_source(const ezkl_program_t* prog, char* out, size_t cap, size_t* len);
/* host-only: the instruction order the sweep will execute (the library re-orders a program for short live ranges: every term is
 * computed right before the Horner step that consumes it; dependencies per intermediate are kept, so the value is the program's);
 * out_code receives n_instr x 8 words in the layout of prog->code */
int ezkl_hip_eval_h_schedule(const ezkl_program_t* prog, uint32_t* out_code);
/* Compile the program's kernel now (or load it from the on-disk cache: $EZKL_HIP_CACHE_DIR, ~/.cache/ezkl_hip) without running it:
 * columns / constants / challenges are not read.  A key generator calls it for the circuit's quotient program, so that the first
 * prove of a new circuit -- in this or a later process -- does not wait for hiprtc (seconds for an ezkl-sized program). */
int ezkl_hip_eval_h_prepare(const ezkl_program_t* prog);
/* how this process obtained its sweep kernels so far: compiled by hiprtc, loaded from the on-disk cache, found in memory */
int ezkl_hip_eval_h_jit_stats(uint64_t* compiled, uint64_t* from_disk, uint64_t* memory_hits);

/* ---- mock prover: report the failing constraints instead of folding them into a quotient or a count (halo2 MockProver::verify) ----
 * Every call appends 16-byte records {kind, index, sub, row} to records_dev through a cursor: counters_dev[0] (device u64, zeroed by the
 * caller for a fresh list) is ADDED the number of failures found, and failure i of the call goes to records_dev[cursor_before + i] when that
 * is below cap -- failures past cap are counted, never written (records_dev may be NULL when cap = 0).  The order of the records is
 * unspecified.  The calls return after their kernels have run. */
typedef struct { uint32_t kind, index, sub, row; } ezkl_check_record_t;   /* kind 1 gate, 2 lookup, 3 copy */
/* Gate check: the program runs with ext_k == k on the Lagrange rows themselves (a rotation is a row offset, indices wrap mod 2^k).  For
 * every row in [row_lo, row_hi) and every listed intermediate j (written by the program, listed once) whose final value is not zero:
 * {1, j, 0, row}.  JIT-compiled like the sweep (same validation, scheduling and on-disk cache, a cache identity of its own); radix-2^29
 * generators only: EZKL_EVALH_R29=0 gives EZKL_ERR_INVALID. */
int ezkl_hip_eval_check_dev(const ezkl_program_t* prog, const uint32_t* check_slots, uint32_t n_checks, uint32_t row_lo, uint32_t row_hi, void* records_dev,
                            uint32_t cap, void* counters_dev, void* stream);
/* host-only: the source of that check kernel, with the contract of ezkl_hip_eval_h_source */
int ezkl_hip_eval_check_source(const ezkl_program_t* prog, const uint32_t* check_slots, uint32_t n_checks, char* out, size_t cap, size_t* len);
/* Lookup miss rows: the inputs and tables of ezkl_hip_lookup_multiplicity_batch_dev (theta-compressed columns; input j belongs to argument
 * input_lookup[j]).  For every usable row r of an input absent from the usable rows of its table: {2, lookup, input, r}, `input` counting
 * the argument's own inputs from 0.  counters_dev holds 1 + n_lookups u64: the cursor, then per argument the number of its misses (the
 * `missing` of lookup_multiplicity_batch_dev on the same columns). */
int ezkl_hip_lookup_missing_rows_dev(const void* const* inputs_dev, const uint32_t* input_lookup, uint32_t n_inputs, const void* const* tables_dev,
                                     uint32_t n_lookups, uint32_t n_rows, uint32_t usable_rows, void* records_dev, uint32_t cap, void* counters_dev,
                                     void* stream);
/* Copy check: m columns of 2^log_n rows (cols_dev: m device pointers in host memory), cells numbered c 2^log_n + r as in
 * ezkl_hip_permutation_sigma_dev; next_dev (device u32, m 2^log_n entries) = the cycle successor of every cell.  Every cell whose value
 * differs from its successor's (or whose successor lies outside the m columns): {3, c, 0, r}. */
int ezkl_hip_copy_check_dev(const void* const* cols_dev, uint32_t m, const void* next_dev, uint32_t log_n, void* records_dev, uint32_t cap, void* counters_dev,
                            void* stream);

/* ---- multi-GPU: the collectives of the sharded prove path, RCCL over xGMI on the library's device pointers (csrc/comm.hip) ----
 * One process per GPU (ezkl_hip_init picks the device).  The reference has no multi-GPU path (icicle is single-GPU), so
 * these replace nothing: a launcher creates the id on rank 0 (ezkl_hip_comm_unique_id), hands the 128 bytes to every rank by whatever
 * means it has (env, file, MPI, torch.distributed), and every rank calls ezkl_hip_comm_init.  librccl is dlopen'ed on first use.
 * EZKL_ERR_UNSUPPORTED: RCCL cannot be loaded.  MSM partials: gather-then-add (RCCL has no elliptic-curve reduce op). */
int ezkl_hip_comm_unique_id(void* out128);
int ezkl_hip_comm_init(const void* id128, int world, int rank);
int ezkl_hip_comm_info(int* world, int* rank);            /* world = 0: no communicator */
int ezkl_hip_comm_destroy(void);
/* in-place all_gather of a device buffer made of `world` equal slices (rank r wrote slice r): the row-sharded quotient sweep's h */
int ezkl_hip_comm_allgather_dev(void* buf_dev, size_t total_bytes);
/* one commit batch: `count` 64-byte affine Montgomery partial sums (host) -> their sums over all ranks, in place, on every rank */
int ezkl_hip_comm_fold_points(void* points_host, uint32_t count);
/* broadcast of a small host buffer (<= 4096 B) from rank `root`: the OS-entropy ChaCha key of a sharded proof */
int ezkl_hip_comm_broadcast_host(void* buf_host, size_t bytes, int root);
/* all-to-all on device pointers (per-peer byte offsets / lengths): columns transformed by their owner -> the row shards of the sweep */
int ezkl_hip_comm_alltoall_dev(const void* send_dev, const size_t* send_off, const size_t* send_len, void* recv_dev, const size_t* recv_off,
                               const size_t* recv_len);

/* all_gather of small HOST buffers: buf_host holds world x bytes_per_rank bytes, rank r has filled slice r; on return every slice is
 * filled on every rank (the evaluations a rank computed for the polynomials it owns; the chaining values of the permutation chunks) */
int ezkl_hip_comm_allgather_host(void* buf_host, size_t bytes_per_rank);
/* all-to-all with ANY NUMBER of contiguous device segments per peer: sends[i] goes to sends[i].peer, recvs[j] arrives from recvs[j].peer.
 * Per (sender, receiver) pair the segments form ONE byte stream in list order -- the k-th byte this rank sends to peer p is the k-th byte
 * p receives from this rank -- so only the per-pair totals must agree.  A column-sharded prover moves the cosets (or halo-extended row
 * windows) of the columns it transformed to the ranks that sweep those rows with ONE such call.  Wire format: a device gather kernel packs
 * each peer's stream into a slab (rounds of at most EZKL_COMM_SLAB_MB, default 128 MiB, per peer and direction; the same on every rank),
 * ONE ncclSend + ONE ncclRecv per peer and round inside one group (all xGMI links at once), a scatter kernel unpacks.  Bytes to the own
 * rank are copied by the same kernel.  Segments may have any address and length: 16-byte aligned pieces (the prover's field columns) move
 * as vectors, others byte by byte, in the SAME wire format -- which format is used never depends on what one rank sees.  EZKL_COMM_UNPACKED=1
 * (set it on every rank or on none): one ncclSend / ncclRecv per segment (round 3; sizes must then agree pairwise).
 * ezkl_hip_comm_stats: out[0] = exchanges, out[1] / out[2] = bytes sent to / received from other ranks, out[3] = microseconds of host wall
 * time inside the exchanges, out[4] / out[5] = ncclSend / ncclRecv operations issued, out[6] = rounds; reset != 0 clears them. */
/* EZKL_OK when librccl can be loaded (from the directory of the HIP runtime this library is bound to) and exports every entry point the
 * communicator binds; EZKL_ERR_UNSUPPORTED otherwise.  Touches no device and calls nothing in RCCL. */
int ezkl_hip_comm_available(void);
typedef struct { int peer; void* ptr; size_t bytes; } ezkl_comm_seg_t;
int ezkl_hip_comm_alltoallv_dev(const ezkl_comm_seg_t* sends, size_t n_sends, const ezkl_comm_seg_t* recvs, size_t n_recvs);
int ezkl_hip_comm_stats(uint64_t out[8], int reset);
/* The communicator tries itself out -- an all_gather of rank ids, ONE packed all-to-all of odd-sized segments, one fold of partial points,
 * each checked -- and fails with a message on stderr instead of hanging or proving wrongly later.  A collective: every rank calls it.
 * ezkl_hip_comm_init runs it by default (EZKL_COMM_SELFTEST=0 on every rank skips).  Every collective of this section is waited for under a
 * watchdog: past EZKL_COMM_TIMEOUT_S seconds (default 120, 0 = none) the call returns EZKL_ERR_TIMEOUT and the communicator is aborted. */
int ezkl_hip_comm_selftest(void);

/* ---- measurement hooks (used by bench.py; HIP events on the stream the kernels run on) ---- */
/* after an msm/ntt call: average device milliseconds of the dominant kernel of the last call */
int ezkl_hip_last_kernel_ms(const char* which, float* out_ms);
/* sum and count of the device milliseconds of EVERY region `which` recorded since the last reset (each call records into an event pair
 * of its own, a ring of 64 per region): a caller can queue K steps back to back and read their kernel times afterwards, without a host
 * synchronisation inside its timed loop.  Waits for the pairs still in flight.  A region that never ran: sum 0, count 0. */
int ezkl_hip_kernel_ms_stats(const char* which, double* sum_ms, uint64_t* count, int reset);
/* Which pairs a synchronous MSM records is the caller's choice through the environment variable EZKL_HIP_TIMING, read at every call:
 * "all" (default: the chain, "msm", and its dominant kernel, "msm_accumulate"), "kernel" (the dominant kernel only), "none" (which also
 * drops the pair around the passes of ezkl_hip_ntt_dev).  An event record
 * is a barrier packet with a timestamp on the stream: the four of one call cost about 15 us of a 1.31 ms 2^20-point MSM. */
/* microbenchmarks: which = "modmul" (Montgomery products/s), "mad64" (v_mad_u64_u32/s),
 * "copy" (HBM float4 copy bytes/s); result in *out (per second) */
int ezkl_hip_ubench(const char* which, double* out);

/* ---- test hooks ---- */
/* ONE field primitive of csrc/field.hpp or csrc/field29.hpp applied to n rows of operands that are on the device (csrc/fieldprobe.hip):
 * the tests compare every word with big-integer arithmetic at the operands where a carry, a borrow or a conditional subtraction can go
 * wrong.  `name` is "<field>.<primitive>" with field fr / fq (rows of 8 uint32 words) or fr29 / fq29 (rows of 9), e.g. "fr.mul_lazy",
 * "fq29.cond_sub2"; an unknown name is EZKL_ERR_INVALID.  Operand j of row i is the row i of ops_dev[j] (up to 4 operands, unused ones
 * may be NULL), the result is row i of out_dev.  "<field>.live_<product>" probes write the product, then 6 further rows of operand 0
 * (rows i+1 .. i+6 mod n) that were held in registers across the product, then 64 words 0x9e3779b9 * (j + 1) held in scalar registers. */
int ezkl_hip_field_probe_dev(const char* name, const void* const ops_dev[4], void* out_dev, size_t n, void* stream);
/* every name the probe knows, one per line: "<name> <operands> <words per operand row> <words per result row>".  Host only.  *len is the
 * length of the whole list; at most cap - 1 characters and a 0 are written to out (out may be NULL to ask for the length). */
int ezkl_hip_field_probe_names(char* out, size_t cap, size_t* len);

#ifdef __cplusplus
}
#endif
#endif
