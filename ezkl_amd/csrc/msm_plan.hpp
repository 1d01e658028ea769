// msm_plan.hpp -- the host side of one MSM launch chain as integer arithmetic: the window plan, the launch geometry of the chain's kernels and
// the layout of a scratch slab, computed by ONE pure function (msm_plan) from (n, window plan, group size, CU count, occupancy, tuning).
// Plain C++17 without HIP headers: msm.hip launches what this says, tests/cpp/test_msm_plan.cpp holds it to the constraints the kernels rely
// on (LDS sizes, tile sizes, exact tilings of the reduce fields, disjoint and sufficient scratch regions) without a GPU.
#pragma once
#include <cstddef>
#include <cstdint>
#if defined(__HIPCC__) || defined(__HIP__)
#define MSM_HD __host__ __device__
#else
#define MSM_HD
#endif

namespace ezkl {

// (The compile-time variants of rounds 4-5 -- the loop without the one-iteration-ahead loads, the fused "lean" chain, unpack-first, the full
// accumulator reset, conditional gathers -- were measured and removed; their A/B logs are profiles/r05q_msm_ab.log, r05y_msm_ab.log and
// DESIGN.md §4.1.  What is here is the one shipped form.)
static constexpr uint32_t MSM_MAX_PART_BITS = 12;   // <= 4096 partitions in the first sorting pass (1024 up to 2^20 points: msm_part_bits)
static constexpr uint32_t MSM_SPAN_HEAVY = 16;      // buckets cut by more lane boundaries than this are folded by a whole workgroup
static constexpr uint32_t MSM_PART_STAGE = 13312;     // pairs a partition workgroup stages in LDS (104 KiB): 1024 scalars x 13 windows
static constexpr uint32_t MSM_BINSORT_STAGE = 15360;  // payloads a sort workgroup stages in LDS (60 KiB): 2 workgroups per CU
static constexpr uint32_t MSM_HEAVY_CHUNK = 256;     // lane partials folded by one WAVE in the first heavy pass (four serial additions per lane + the wave tree)
static constexpr uint32_t MSM_DIGIT_E = 8;          // serial elements per lane in the first reduce stage
static constexpr uint32_t MSM_LMIN = 8;             // shortest lane of the accumulate kernel
static constexpr uint32_t MSM_MAX_BIG = 64;         // oversized partitions sorted by several workgroups each (the rest: one workgroup)
static constexpr uint32_t MSM_BIG_BLOCKS = 64;      // workgroups per oversized partition
static constexpr uint32_t MSM_BIG_ROWS = 8;         // rows of such workgroups in a launch: row r takes the oversized partitions r, r + 8, ...
static constexpr uint32_t MSM_SCAN_COLS = 4;        // columns of the (tile, partition) table scanned by one workgroup (msm_hist_scan_kernel)
static constexpr size_t MSM_MAX_GROUP = 16;       // MSMs fused into one sequence of launches (gridDim.z)
static constexpr uint32_t MSM_PART_LDS = 144u << 10;      // dynamic LDS the partition kernel may ask for: one workgroup per CU
static constexpr uint32_t MSM_BINSORT_LDS = 96u << 10;    // dynamic LDS the second sorting pass may ask for
static constexpr size_t MSM_POINT_BYTES = 144;    // sizeof(g1x29_t): an XYZZ point of 4 x 9 radix-2^29 limbs

// Window plan: W signed-digit windows covering 254 bits (253-bit magnitudes after the r - s fold + the last carry),
// the first `rem` windows base+1 bits wide, the others base bits.  Balanced widths instead of "c, c, ..., short top
// window": a 14-bit top window under c = 20 pours 128 extra pairs into each of 2^13 buckets, which then get cut by
// several lane boundaries of the accumulate kernel; with 7 x 20 + 6 x 19 bits no bucket outgrows a lane.
struct WinPlan {
    uint32_t W, base, rem;
    MSM_HD uint32_t width(uint32_t w) const { return base + (w < rem ? 1u : 0u); }
    MSM_HD uint32_t offset(uint32_t w) const { return w * base + (w < rem ? w : rem); }
    MSM_HD uint32_t cmax() const { return base + (rem ? 1u : 0u); }
};
inline WinPlan pick_plan(size_t n) {
    // cost model in point additions: n*W bucket additions + ~4 per bucket for the reduce phase (2^(cmax-1) buckets);
    // ties go to the smaller W (fewer gathers, smaller table).  n = 2^20: W = 13 (7 x 20 + 6 x 19 bits, 26 pairs/bucket).
    WinPlan best{0, 0, 0};
    double best_cost = 0;
    for (uint32_t W = 10; W <= 127; W++) {
        WinPlan p{W, 254 / W, 254 % W};
        if (p.cmax() > 23) continue;
        const double cost = (double)n * W + 4.0 * (double)((size_t)1 << (p.cmax() - 1));
        if (!best.W || cost < best_cost) { best = p; best_cost = cost; }
    }
    return best;
}

// ---- reduce: sum_pos weight(pos) * B_pos ---------------------------------------------------------
// A bucket position splits into three bit-fields A (lowest), B, C; its weight is 1 + dA*2^wsA + dB*2^wsB +
// dC*2^wsC.  So the weighted sum is TOTAL + sum over fields of 2^ws * sum_d d * S_field[d], with S_field[d] the
// plain sum of the buckets whose field equals d.  S_A comes from column sums; S_B and S_C come from the row
// sums T[dC,dB] = sum_dA B: two passes over the buckets, each a shallow reduction (no running sums, whose
// dependent chains are latency-bound on a GPU), then per-bit plane sums; the final Horner over <= 22 planes
// runs on the host.
struct ReduceGeom {
    uint32_t wA, wB, wC;          // field widths (pos bits: A = [0,wA), B = [wA,wA+wB), C = rest)
    uint32_t wsA, wsB, wsC;       // weight shifts of the fields
    uint32_t EA, GA, ET, GT;      // serial elements per lane / groups for column sums (A) and row sums (T)
};

// what the environment may override (msm.hip: msm_tuning); the defaults are the measured optimum
struct MsmTuning {
    uint32_t L_override = 0;                  // host lane length of the accumulate kernel; 0: chosen by msm_plan
    uint32_t E = MSM_DIGIT_E;                 // a power of two <= 1024
    uint32_t lmin = MSM_LMIN;                 // device-side floor of the lane length (columns with few non-zero digits)
    uint32_t span_heavy = MSM_SPAN_HEAVY;     // the cut count above which a bucket takes the heavy path
};

// everything msm_enqueue knows before it touches the device:
//   W, bits, nb        windows, bucket bits, buckets;  npairs: the (bucket, payload) pairs the launches are sized for, n * W
//   PB, LB, NP, NQ     partition / in-partition bucket bits, partitions, partitions + bucket 0's own
//   L, nlanes          host lane length and lanes of the accumulate kernel
//   per_block          scalars per sort tile = threads of a partition workgroup;  sgrid: tiles;  pgrid: persistent partition workgroups
//   part_lds           the partition kernel's dynamic LDS bytes
//   hb, cb             workgroups of the two heavy passes (heavy2, heavy1);  r1grid, r2grid: workgroups of reduce1 / reduce2
//   lanesA, lanesT     reduce2: lanes of a wave per output;  blocksA: its workgroups of the A half
//   o                  byte offsets of the scratch regions inside a slab, each 256-byte aligned
//   zero_bytes         hcnt, btot, planes: the run the histogram kernel zeroes
//   slab_bytes         one MSM's scratch;  bstride: distance between the slabs of a fused group (0: a single MSM)
struct MsmPlan {
    uint32_t W, bits, nb, PB, LB, NP, NQ, L, nlanes;
    size_t npairs, per_block, part_lds;
    unsigned sgrid, pgrid, hb, cb, r1grid, r2grid;
    ReduceGeom rg;
    uint32_t nA, nT, n_partA, n_partT, nplanes, lanesA, lanesT, blocksA;
    struct Off { size_t ent, vals, offs, pcnt, pbase, wghist, heavy, chunks, hcnt, btot, planes, bflag, blist, boff, lfirst, bkt, head, tail, partA, partT, SA, T; } o;
    size_t zero_bytes, slab_bytes, bstride;
};

inline MsmPlan msm_plan(size_t n, WinPlan wp, size_t count, int num_cus, int acc_blocks_per_cu, const MsmTuning& tu) {
    MsmPlan p{};
    auto cdiv = [](size_t a, size_t b) { return (unsigned)((a + b - 1) / b); };
    const uint32_t W = p.W = wp.W, bits = p.bits = wp.cmax() - 1;
    const uint32_t nb = p.nb = 1u << bits;
    const size_t npairs = p.npairs = n * W;
    // partitions of the first sorting pass: 1024, or as many more (<= 4096) as it takes to keep a partition inside the second pass's LDS
    // stage -- beyond 2^20 points a partition of the 1024 outgrew it and the second pass fell back to scattered stores (0.9 of the 6 ms of
    // a 2^22-point MSM: profiles/r06u_size_sweep.log, tools/msm22_profile.py)
    uint32_t PB = bits < 10 ? bits : 10;
    while (PB < bits && PB < MSM_MAX_PART_BITS && (npairs >> PB) > (size_t)MSM_BINSORT_STAGE * 9 / 10) PB++;
    const uint32_t LB = p.LB = bits - PB, NP = p.NP = 1u << PB;
    const uint32_t NQ = p.NQ = NP + 1;                   // + bucket 0's own partition (msm_part_of)
    p.PB = PB;
    // ---- lane length for the accumulate kernel: fill the resident lanes an integer number of times ----
    const size_t resident = (size_t)acc_blocks_per_cu * 256 * num_cus;
    // 40..80 pairs per lane at 2^20 points: few cut buckets, whole waves of work.  Larger MSMs have more pairs per BUCKET (104 at 2^22), and a lane
    // shorter than a bucket cuts every bucket several times (the boundary fold was 0.52 of a 2^22-point MSM's 6 ms): the lanes grow with the load
    const size_t load = npairs >> bits, per_lane = load * 9 / 10 > 40 ? load * 9 / 10 : 40;
    size_t rounds = npairs / (resident * per_lane);
    if (rounds < 1) rounds = 1;
    uint32_t L = (uint32_t)((npairs + resident * rounds - 1) / (resident * rounds));
    if (L < 8) L = 8;
    if (tu.L_override) L = tu.L_override;
    p.L = L;
    const uint32_t nlanes = p.nlanes = cdiv(npairs, L);
    // ---- field geometry of the reduce phase (positions: pos = (bucket & (NP-1)) << LB | bucket >> PB) ----
    ReduceGeom& rg = p.rg;
    if (LB > 0) {
        rg.wA = LB; rg.wsA = PB;                          // A = high bucket bits
        rg.wB = (PB + 1) / 2; rg.wsB = 0;                 // B, C = low bucket bits
        rg.wC = PB - rg.wB; rg.wsC = rg.wB;
    } else {                                              // small MSM: pos == bucket
        rg.wA = (bits + 2) / 3; rg.wsA = 0;
        rg.wB = (bits - rg.wA + 1) / 2; rg.wsB = rg.wA;
        rg.wC = bits - rg.wA - rg.wB; rg.wsC = rg.wA + rg.wB;
    }
    {
        const uint32_t rows = 1u << (rg.wB + rg.wC), cols = 1u << rg.wA, E = tu.E;
        rg.EA = rows < E ? rows : E; rg.GA = rows / rg.EA;
        rg.ET = cols < E ? cols : E; rg.GT = cols / rg.ET;
    }
    const uint32_t nA = p.nA = 1u << rg.wA, nT = p.nT = 1u << (rg.wB + rg.wC);
    const uint32_t n_partA = p.n_partA = nA * rg.GA, n_partT = p.n_partT = nT * rg.GT;
    const uint32_t nplanes = p.nplanes = 1 + bits;
    // ---- sort geometry: sgrid workgroups, each owning per_block consecutive scalars ----
    // (one scalar per thread of the partition pass; all of a workgroup's pairs must fit its LDS staging area)
    size_t per_block = MSM_PART_STAGE / W / 64 * 64;
    {
        const size_t lds_words = MSM_PART_LDS / 4, fixed = 3 * ((size_t)NQ + 1);       // the partition kernel's 144 KiB: three arrays of NQ + 1 words, then 2 W words per scalar
        const size_t fit = lds_words > fixed ? (lds_words - fixed) / (2 * (size_t)W) / 64 * 64 : 64;
        if (per_block > fit) per_block = fit;
    }
    if (per_block > 1024) per_block = 1024;
    if (per_block < 64) per_block = 64;
    p.per_block = per_block;
    const unsigned sgrid = p.sgrid = cdiv(n, per_block);
    // persistent: one workgroup per CU (its 144 KiB of LDS leave room for no second one) walks the tiles
    p.pgrid = sgrid < (unsigned)num_cus ? sgrid : (unsigned)num_cus;
    p.part_lds = (3 * ((size_t)NQ + 1) + 2 * per_block * W) * 4;
    // ---- the heavy passes: four buckets / four chunks (waves) per workgroup ----
    {
        const size_t max_heavy = nlanes / tu.span_heavy + 1, max_chunks = nlanes / MSM_HEAVY_CHUNK + max_heavy;
        const size_t heavy_wgs = (max_heavy + 3) / 4, chunk_wgs = (max_chunks + 3) / 4;
        p.hb = (unsigned)(heavy_wgs < (size_t)num_cus * 4 ? heavy_wgs : (size_t)num_cus * 4);
        p.cb = (unsigned)(chunk_wgs < (size_t)num_cus * 4 ? chunk_wgs : (size_t)num_cus * 4);
    }
    // ---- reduce: the lane counts of reduce2 are chosen so that the launch has at most one wave per SIMD (msm_reduce2_kernel) ----
    {
        p.r1grid = cdiv(n_partA > n_partT ? n_partA : n_partT, 256);
        auto pow2_le = [](uint32_t x) { uint32_t q = 1; while (q * 2 <= x) q *= 2; return q; };
        uint32_t lanesA = pow2_le(rg.GA < 64 ? rg.GA : 64), lanesT = pow2_le(rg.GT < 64 ? rg.GT : 64);
        auto waves = [&](uint32_t nout, uint32_t lanes) { return cdiv(nout, 64 / lanes); };
        while (waves(nA, lanesA) + waves(nT, lanesT) > (unsigned)num_cus * 4 && (lanesA > 1 || lanesT > 1)) {
            if (lanesT > 1 && waves(nT, lanesT) >= waves(nA, lanesA)) lanesT >>= 1; else if (lanesA > 1) lanesA >>= 1; else lanesT >>= 1;
        }
        p.lanesA = lanesA; p.lanesT = lanesT;
        p.blocksA = waves(nA, lanesA);
        p.r2grid = p.blocksA + waves(nT, lanesT);
    }
    // ---- carve scratch ----
    size_t off = 0;
    auto carve = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    MsmPlan::Off& o = p.o;
    o.ent = carve(npairs * 8); o.vals = carve(npairs * 4); o.offs = carve(((size_t)nb + 1) * 4);
    o.pcnt = carve((NQ + 1) * 4); o.pbase = carve((NQ + 1) * 4); o.wghist = carve((size_t)sgrid * NQ * 4);
    o.heavy = carve((size_t)nb * 4); o.chunks = carve(((size_t)nlanes + 1) * 4);
    const size_t nbins = (size_t)1 << LB;
    // ONE region that starts every chain at zero: the counters (hcnt[0] heavy buckets, [1] chunks, [2] oversized partitions), the bin
    // totals of the multi-workgroup sort, the planes
    o.hcnt = carve(256); o.btot = carve(MSM_MAX_BIG * nbins * 4); o.planes = carve((size_t)nplanes * MSM_POINT_BYTES);
    p.zero_bytes = off - o.hcnt;
    o.bflag = carve((size_t)NP * 4); o.blist = carve(MSM_MAX_BIG * 4); o.boff = carve((size_t)MSM_MAX_BIG * MSM_BIG_BLOCKS * nbins * 4);
    o.lfirst = carve((size_t)nlanes * 4);
    o.bkt = carve((size_t)nb * MSM_POINT_BYTES);
    o.head = carve((size_t)nlanes * MSM_POINT_BYTES); o.tail = carve((size_t)nlanes * MSM_POINT_BYTES);
    o.partA = carve((size_t)n_partA * MSM_POINT_BYTES); o.partT = carve((size_t)n_partT * MSM_POINT_BYTES);
    o.SA = carve((size_t)nA * MSM_POINT_BYTES); o.T = carve((size_t)nT * MSM_POINT_BYTES);
    p.slab_bytes = off;
    p.bstride = count > 1 ? off : 0;                      // every MSM of the group owns one slab of this layout
    return p;
}

// ---- an MSM WITHOUT window tables (msm.hip: msm_once_run) ------------------------------------------------------------------------
// sum_i s_i P_i = sum_w 2^offset(w) * S_w with S_w = sum_i d_{w,i} P_i: every window is an MSM of its own over the raw points -- the chain
// above with the points as a one-level "table", the pairs of ONE window, n pairs instead of n * W -- and the windows are the members of fused
// groups (gridDim.z), because they read the same scalar column.  The host combines the S_w (msm_once_finish).
// Cost model in point additions: every window has a bucket set of its own, so W * (n + 4 * 2^(cmax-1)), plus what a SEQUENCE OF LAUNCHES
// costs when W outgrows one fused group: 14 launches and their latency-bound tails, measured at 0.3-0.5 ms (2^14 points: 0.80 ms as 12 + 12
// windows, 0.49 ms as 16; 2^16: 1.09 ms as 11 + 11, 0.58 ms as 16 -- DESIGN.md §4.1), which is 2^22 additions at the ~7 per ns the path
// sustains at 2^20 points.  So in practice a plan is 12 .. 16 windows in ONE sequence, and narrower windows than pick_plan's: 2^20 points:
// W = 16 (14 x 16 + 2 x 15 bits) where the table path has 13 windows of 20 / 19 bits.
static constexpr size_t MSM_ONCE_CHAIN_COST = (size_t)1 << 22;        // one sequence of launches, in point additions
static constexpr uint32_t MSM_ONCE_MAX_W = 127;                       // most windows of a plan (two bits each): the landing buffer has a block for each
static constexpr size_t MSM_ONCE_SCRATCH_CAP =(size_t)4 << 30;       // the slabs of one fused group stay below this (fewer windows per group beyond it)
inline WinPlan pick_plan_once(size_t n) {
    WinPlan best{0, 0, 0};
    double best_cost = 0;
    for (uint32_t W = 12; W <= MSM_ONCE_MAX_W; W++) {     // 254 bits in windows of at most 23 (msm_recode's bit buffer): at least 12 of them
        WinPlan p{W, 254 / W, 254 % W};
        if (p.cmax() > 23) continue;
        const double groups = (double)((W + MSM_MAX_GROUP - 1) / MSM_MAX_GROUP);
        const double cost = (double)W * ((double)n + 4.0 * (double)((size_t)1 << (p.cmax() - 1))) + groups * (double)MSM_ONCE_CHAIN_COST;
        if (!best.W || cost < best_cost) { best = p; best_cost = cost; }
    }
    return best;
}
// the launch plan of a table-free MSM:
//   wp             the W windows the scalars are recoded into (pick_plan_once)
//   chain          ONE window's chain: msm_plan for n pairs (a plan of one window as wide as wp's widest), `group` slabs bstride apart;
//                  the lanes are sized for the pairs of the whole group, which share the device
//   group, ngroups windows per sequence of launches (<= MSM_MAX_GROUP; fewer when their slabs would outgrow MSM_ONCE_SCRATCH_CAP) and
//                  sequences: sequence g serves the windows [g * group, min(W, (g + 1) * group)) and reuses the slabs
//   o_points       the points in the accumulate kernel's form (R' = 2^261), n x 64 bytes, shared by all windows;  o_slabs: the first slab
//   bytes          the whole scratch
struct MsmOncePlan {
    WinPlan wp;
    MsmPlan chain;
    size_t group, ngroups, o_points, o_slabs, bytes;
};
inline MsmOncePlan msm_plan_once(size_t n, int num_cus, int acc_blocks_per_cu, const MsmTuning& tu) {
    MsmOncePlan q{};
    q.wp = pick_plan_once(n);
    const WinPlan one{1, q.wp.cmax(), 0};                 // bits = cmax - 1, npairs = n: a narrower window of wp uses the low half of the buckets
    size_t group = q.wp.W < MSM_MAX_GROUP ? q.wp.W : MSM_MAX_GROUP;
    for (;;) {
        q.ngroups = (q.wp.W + group - 1) / group;
        q.group = group = (q.wp.W + q.ngroups - 1) / q.ngroups;   // balanced: 13 windows under the cap go as 5 + 5 + 3, not 6 + 6 + 1
        MsmTuning t = tu;
        if (!t.L_override) {                              // msm_plan's lane rule, for the group's pairs
            const size_t resident = (size_t)acc_blocks_per_cu * 256 * num_cus, total = n * group;
            const size_t load = n >> (one.cmax() - 1), per_lane = load * 9 / 10 > 40 ? load * 9 / 10 : 40;
            size_t rounds = total / (resident * per_lane);
            if (rounds < 1) rounds = 1;
            const size_t L = (total + resident * rounds - 1) / (resident * rounds);
            t.L_override = (uint32_t)(L < 8 ? 8 : L);
        }
        q.chain = msm_plan(n, one, group, num_cus, acc_blocks_per_cu, t);
        if (group == 1 || group * q.chain.slab_bytes <= MSM_ONCE_SCRATCH_CAP) break;
        group--;                                          // (the lanes, and with them a slab, depend on the group: sized again)
    }
    q.o_points = 0;
    q.o_slabs = (n * 64 + 255) & ~(size_t)255;
    q.bytes = q.o_slabs + group * q.chain.slab_bytes;
    return q;
}

}  // namespace ezkl
