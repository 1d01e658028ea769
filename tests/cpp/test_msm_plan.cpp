// The MSM's host-side launch plan (ezkl_amd/csrc/msm_plan.hpp: pick_plan and msm_plan) held to what the kernels of the chain rely on, without a
// device: a stand-alone program, built by tests/test_msm_plan_cpp.py under AddressSanitizer and UndefinedBehaviorSanitizer.
//
// Sweep: every n in 1 .. 8192; 2^k - 1, 2^k, 2^k + 1 for k = 13 .. 26; 2^18 + 1025 and 212 993 (the sizes of tests/test_gpu_msm_front.py); 3000
// random n below 2^24; devices of 1, 8, 64, 256 and 304 CUs with 1, 2 or 3 resident accumulate workgroups per CU; groups of 1, 2 and 16
// MSMs under the default tuning, and single MSMs under L_override 8 / 64, E 1 / 1024, lmin 1 / 64, span_heavy 1 / 4096.
// For every plan (the names are MsmPlan's):
//   windows    wp.offset(W) == 254, cmax <= 23, bits == cmax - 1, nb == 2^bits, npairs == n * W
//   partitions PB + LB == bits, PB <= MSM_MAX_PART_BITS, NP == 2^PB, NQ == NP + 1
//   tiles      per_block a multiple of 64 in 64 .. 1024; per_block * W <= MSM_PART_STAGE unless per_block == 64; part_lds is three arrays of
//              NQ + 1 words and 2 W words per scalar, within MSM_PART_LDS; the second pass's stage within MSM_BINSORT_LDS;
//              sgrid * per_block >= n > (sgrid - 1) * per_block; pgrid == min(sgrid, num_cus)
//   lanes      L >= 8 (the override: as given); nlanes * L >= npairs > (nlanes - 1) * L
//   heavy      1 <= hb, cb <= 4 * num_cus
//   reduce     wA + wB + wC == bits; EA * GA == 2^(wB + wC), ET * GT == 2^wA; nA, nT, n_partA, n_partT, nplanes follow; the weight shifts are a
//              permutation of the field offsets; reduce1's grid covers both halves; lanesA, lanesT are powers of two <= 64 and <= GA, GT;
//              blocksA and r2grid are the waves those lane counts need; r2grid <= 4 * num_cus whenever a lane count could still be halved
//   scratch    every region starts on a 256-byte boundary; the regions, each as large as what the launch that writes it is given, are pairwise
//              disjoint and end inside slab_bytes; the zeroed run is exactly hcnt, btot, planes, contiguous, a multiple of 4 bytes, and nothing
//              else lies inside it; slab_bytes is the (aligned) end of the last region; bstride == (count > 1 ? slab_bytes : 0)
// and the table of tests/test_gpu_msm_front.py's sizes on a 256-CU device with 3 resident workgroups per CU is pinned.
#include "msm_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace ezkl;

struct Case {
    size_t n, count;
    int num_cus, occ;
    MsmTuning tu;
};
static size_t g_checks = 0;
[[noreturn]] static void fail(const Case& c, const char* what) {
    printf("FAILED: %s\n  at n=%zu count=%zu num_cus=%d acc_blocks_per_cu=%d L_override=%u E=%u lmin=%u span_heavy=%u\n", what, c.n, c.count, c.num_cus, c.occ,
           c.tu.L_override, c.tu.E, c.tu.lmin, c.tu.span_heavy);
    exit(1);
}
#define CHECK(cond) do { g_checks++; if (!(cond)) fail(c, #cond); } while (0)

static size_t al(size_t x) { return (x + 255) & ~(size_t)255; }
static size_t cdiv(size_t a, size_t b) { return (a + b - 1) / b; }
static bool pow2(uint32_t x) { return x && !(x & (x - 1)); }

struct Region {
    const char* name;
    size_t off, need;      // need: the bytes the kernels are entitled to, from what msm_enqueue passes them
};

static void check(const Case& c) {
    const WinPlan wp = pick_plan(c.n);
    const MsmPlan p = msm_plan(c.n, wp, c.count, c.num_cus, c.occ, c.tu);
    const size_t cus4 = (size_t)c.num_cus * 4;
    // windows
    CHECK(wp.W >= 10 && wp.offset(wp.W) == 254);
    CHECK(wp.cmax() <= 23);
    CHECK(p.W == wp.W && p.bits == wp.cmax() - 1 && p.nb == 1u << p.bits && p.npairs == c.n * wp.W);
    // partitions
    CHECK(p.PB + p.LB == p.bits);
    CHECK(p.PB <= MSM_MAX_PART_BITS);
    CHECK(p.NP == 1u << p.PB);
    CHECK(p.NQ == p.NP + 1);
    // tiles
    CHECK(p.per_block % 64 == 0 && p.per_block >= 64 && p.per_block <= 1024);
    CHECK(p.per_block * p.W <= MSM_PART_STAGE || p.per_block == 64);
    CHECK(p.part_lds == (3 * ((size_t)p.NQ + 1) + 2 * p.per_block * p.W) * 4);
    CHECK(p.part_lds <= MSM_PART_LDS);
    CHECK((size_t)MSM_BINSORT_STAGE * 4 <= MSM_BINSORT_LDS);
    CHECK((size_t)p.sgrid * p.per_block >= c.n && c.n > ((size_t)p.sgrid - 1) * p.per_block);
    CHECK(p.pgrid == std::min<size_t>(p.sgrid, (size_t)c.num_cus));
    // lanes
    CHECK(c.tu.L_override ? p.L == c.tu.L_override : p.L >= 8);
    CHECK((size_t)p.nlanes * p.L >= p.npairs && p.npairs > ((size_t)p.nlanes - 1) * p.L);
    // heavy passes
    CHECK(p.hb >= 1 && p.hb <= cus4 && p.cb >= 1 && p.cb <= cus4);
    // reduce
    const ReduceGeom& g = p.rg;
    CHECK(g.wA + g.wB + g.wC == p.bits);
    CHECK((size_t)g.EA * g.GA == (size_t)1 << (g.wB + g.wC));
    CHECK((size_t)g.ET * g.GT == (size_t)1 << g.wA);
    CHECK(p.nA == 1u << g.wA && p.nT == 1u << (g.wB + g.wC) && p.n_partA == p.nA * g.GA && p.n_partT == p.nT * g.GT && p.nplanes == 1 + p.bits);
    {   // every bit of a bucket id is weighted exactly once: the three fields, shifted, tile [0, bits)
        uint64_t seen = 0;
        const uint32_t w[3] = {g.wA, g.wB, g.wC}, ws[3] = {g.wsA, g.wsB, g.wsC};
        bool ok = true;
        for (int f = 0; f < 3; f++)
            for (uint32_t j = 0; j < w[f]; j++) {
                ok = ok && ws[f] + j < p.bits && !(seen >> (ws[f] + j) & 1);
                seen |= (uint64_t)1 << (ws[f] + j);
            }
        CHECK(ok && seen == ((uint64_t)1 << p.bits) - 1);
    }
    CHECK((size_t)p.r1grid * 256 >= std::max(p.n_partA, p.n_partT) && ((size_t)p.r1grid - 1) * 256 < std::max(p.n_partA, p.n_partT));
    CHECK(pow2(p.lanesA) && p.lanesA <= 64 && p.lanesA <= g.GA);
    CHECK(pow2(p.lanesT) && p.lanesT <= 64 && p.lanesT <= g.GT);
    CHECK(p.blocksA == cdiv(p.nA, 64 / p.lanesA));
    CHECK(p.r2grid == p.blocksA + cdiv(p.nT, 64 / p.lanesT));
    CHECK(p.r2grid <= cus4 || (p.lanesA == 1 && p.lanesT == 1));
    // scratch
    const size_t PT = MSM_POINT_BYTES, nbins = (size_t)1 << p.LB;
    std::vector<Region> r = {
        {"ent", p.o.ent, p.npairs * 8},                                  // (bucket, payload) pairs: partition pass
        {"vals", p.o.vals, p.npairs * 4},                                // sorted payloads
        {"offs", p.o.offs, ((size_t)p.nb + 1) * 4},                      // bucket offsets, offs[nb] = the number of pairs
        {"pcnt", p.o.pcnt, (size_t)p.NQ * 4},                            // hist_scan: one total per partition
        {"pbase", p.o.pbase, ((size_t)p.NQ + 1) * 4},                    // part_scan: part_base[NQ] = the number of pairs
        {"wghist", p.o.wghist, (size_t)p.sgrid * p.NQ * 4},              // one row of NQ counts per tile
        {"heavy", p.o.heavy, std::min<size_t>(p.nb, p.nlanes / MSM_HEAVY_CHUNK + 1) * 4},      // buckets cut more than MSM_HEAVY_CHUNK times, each once
        {"chunks", p.o.chunks, (size_t)p.nlanes * 4},                    // at most one entry per lane boundary
        {"hcnt", p.o.hcnt, 3 * 4},                                       // heavy buckets, chunks, oversized partitions
        {"btot", p.o.btot, MSM_MAX_BIG * nbins * 4},
        {"planes", p.o.planes, (size_t)p.nplanes * PT},
        {"bflag", p.o.bflag, (size_t)p.NP * 4},
        {"blist", p.o.blist, MSM_MAX_BIG * 4},
        {"boff", p.o.boff, (size_t)MSM_MAX_BIG * MSM_BIG_BLOCKS * nbins * 4},
        {"lfirst", p.o.lfirst, (size_t)p.nlanes * 4},
        {"bkt", p.o.bkt, (size_t)p.nb * PT},
        {"head", p.o.head, (size_t)p.nlanes * PT},
        {"tail", p.o.tail, (size_t)p.nlanes * PT},
        {"partA", p.o.partA, (size_t)p.n_partA * PT},
        {"partT", p.o.partT, (size_t)p.n_partT * PT},
        {"SA", p.o.SA, (size_t)p.nA * PT},
        {"T", p.o.T, (size_t)p.nT * PT},
    };
    std::sort(r.begin(), r.end(), [](const Region& a, const Region& b) { return a.off < b.off; });
    bool aligned = true, disjoint = true;
    for (size_t i = 0; i < r.size(); i++) {
        aligned = aligned && r[i].off % 256 == 0;
        disjoint = disjoint && r[i].off + r[i].need <= (i + 1 < r.size() ? r[i + 1].off : p.slab_bytes);
    }
    CHECK(aligned);
    CHECK(disjoint);          // sorted by offset: every region ends before the next one starts, the last one inside the slab
    CHECK(p.slab_bytes == r.back().off + al(r.back().need));
    CHECK(p.bstride == (c.count > 1 ? p.slab_bytes : 0));
    // the zeroed run: hcnt, btot, planes and nothing else
    CHECK(p.o.btot == p.o.hcnt + 256 && p.o.planes == p.o.btot + al(MSM_MAX_BIG * nbins * 4));
    CHECK(p.zero_bytes == p.o.planes + al((size_t)p.nplanes * PT) - p.o.hcnt && p.zero_bytes % 4 == 0 && p.zero_bytes / 4 <= 0xffffffffu);
    bool alone = true;
    for (const Region& x : r)
        if (x.off != p.o.hcnt && x.off != p.o.btot && x.off != p.o.planes) alone = alone && (x.off + x.need <= p.o.hcnt || x.off >= p.o.hcnt + p.zero_bytes);
    CHECK(alone);
}

// the plans tests/test_gpu_msm_front.py runs at, on a 256-CU device with 3 resident accumulate workgroups per CU
static void table() {
    struct Row { size_t n; uint32_t W; size_t tile; unsigned tiles; };
    const Row rows[] = {{1, 64, 192, 1}, {255, 29, 448, 1}, {512, 26, 512, 1}, {513, 26, 512, 2}, {1024, 24, 512, 2}, {1025, 24, 512, 3},
                        {4097, 20, 640, 7}, {(1u << 18) + 1025, 15, 832, 317}};
    for (const Row& w : rows) {
        const Case c{w.n, 1, 256, 3, MsmTuning()};
        const MsmPlan p = msm_plan(w.n, pick_plan(w.n), 1, 256, 3, c.tu);
        CHECK(p.W == w.W && p.per_block == w.tile && p.sgrid == w.tiles);
    }
    const Case c{(size_t)1 << 20, 1, 256, 3, MsmTuning()};
    const WinPlan wp = pick_plan(c.n);
    CHECK(wp.W == 13 && wp.base == 19 && wp.rem == 7 && wp.width(6) == 20 && wp.width(7) == 19);     // 7 x 20 + 6 x 19 bits
    CHECK(msm_plan(c.n, wp, 1, 256, 3, c.tu).NP == 1024);
    const Case d{212993, 1, 256, 3, MsmTuning()};                                                    // the smallest size with a 257th tile
    { const Case& c = d; CHECK(msm_plan(d.n, pick_plan(d.n), 1, 256, 3, d.tu).sgrid == 257 && msm_plan(d.n - 1, pick_plan(d.n - 1), 1, 256, 3, d.tu).sgrid == 256); }
}

int main() {
    std::vector<size_t> ns;
    for (size_t n = 1; n <= 8192; n++) ns.push_back(n);
    for (int k = 13; k <= 26; k++)
        for (int d = -1; d <= 1; d++) ns.push_back(((size_t)1 << k) + d);
    ns.push_back((1u << 18) + 1025);
    ns.push_back(212993);
    std::mt19937_64 rng(13);
    for (int i = 0; i < 3000; i++) ns.push_back(1 + rng() % ((1u << 24) - 1));
    std::vector<MsmTuning> tus(9);
    tus[1].L_override = 8; tus[2].L_override = 64; tus[3].E = 1; tus[4].E = 1024; tus[5].lmin = 1; tus[6].lmin = 64; tus[7].span_heavy = 1; tus[8].span_heavy = 4096;
    const int cus[] = {1, 8, 64, 256, 304}, occ[] = {1, 2, 3};
    size_t plans = 0;
    table();
    for (size_t n : ns)
        for (int cu : cus)
            for (int o : occ)
                for (size_t t = 0; t < tus.size(); t++)
                    for (size_t count : {(size_t)1, (size_t)2, (size_t)16}) {
                        if (t && count > 1) continue;
                        check(Case{n, count, cu, o, tus[t]});
                        plans++;
                    }
    printf("all checks passed: %zu sizes, %zu plans, %zu checks\n", ns.size(), plans, g_checks);
    return 0;
}
