// The plan of the G2 MSM (ezkl_amd/csrc/msm_plan.hpp: pick_plan_g2, msm_plan_g2) held to what g2.hip relies on, for n = 1 .. 2^20 at the
// powers of two and their neighbours and for several device sizes: windows that cover 254 bits, buckets that hold every digit, the
// one-level form of the sort front end (position = bucket), groups that fit a launch, and scratch regions that are disjoint and sufficient.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "msm_plan.hpp"
using namespace ezkl;

#define CHECK(c)                                                                                   \
    do {                                                                                           \
        if (!(c)) { std::printf("FAILED %s (n = %zu, line %d)\n", #c, n, __LINE__); std::exit(1); } \
    } while (0)

int main() {
    std::vector<size_t> ns;
    for (unsigned k = 0; k <= 20; k++)
        for (long d = -1; d <= 1; d++) {
            const long v = (1l << k) + d;
            if (v >= 1 && v <= (1l << 20)) ns.push_back((size_t)v);
        }
    const int cus[] = {1, 64, 256, 304};
    for (size_t n : ns)
        for (int num_cus : cus)
            for (int occ = 1; occ <= 3; occ++) {
                const MsmG2Plan q = msm_plan_g2(n, num_cus, occ, MsmTuning{});
                const WinPlan& wp = q.wp;
                CHECK(wp.W >= MSM_G2_MIN_W && wp.W <= MSM_G2_MAX_W && wp.base >= 1);
                uint32_t bits = 0;
                for (uint32_t w = 0; w < wp.W; w++) {
                    CHECK(wp.width(w) >= 1 && wp.width(w) <= wp.cmax() && wp.offset(w) == bits);
                    CHECK(((size_t)1 << (wp.width(w) - 1)) <= q.nb);          // |digit| - 1 < nb
                    bits += wp.width(w);
                }
                CHECK(bits == 254);
                CHECK(q.nb == (1u << (wp.cmax() - 1)) && q.nb <= 1024 && q.chain.nb == q.nb);
                CHECK(q.chain.LB == 0 && q.chain.NP == q.nb);                 // position = bucket: the G2 reduce weighs position b as b + 1
                CHECK(q.chain.npairs == n && q.chain.W == 1);
                CHECK(q.group >= 1 && q.group <= MSM_MAX_GROUP && q.group * q.ngroups >= wp.W && q.group * (q.ngroups - 1) < wp.W);
                CHECK(q.chain.bstride == q.chain.slab_bytes && q.chain.slab_bytes % 256 == 0);
                CHECK((size_t)q.nseg * MSM_G2_SEG >= q.nb && (size_t)(q.nseg - 1) * MSM_G2_SEG < q.nb);
                CHECK(q.long_run >= 2 * MSM_G2_LONG_THREADS && q.long_blocks >= 1 && q.long_blocks <= q.nb);
                CHECK(q.chain.o.heavy + (size_t)q.nb * 4 <= q.chain.slab_bytes);  // the long-run list: one word per bucket inside a slab
                const size_t beg[] = {q.o_slabs, q.o_bkt, q.o_seg, q.o_win, q.o_out, q.bytes};
                const size_t len[] = {q.group * q.chain.slab_bytes, q.group * q.nb * MSM_G2_POINT_BYTES, q.group * q.nseg * 2 * MSM_G2_POINT_BYTES,
                                      wp.W * MSM_G2_POINT_BYTES, 128};
                CHECK(beg[0] == 0);
                for (int r = 0; r < 5; r++) CHECK(beg[r] % 256 == 0 && beg[r] + len[r] <= beg[r + 1]);
            }
    const MsmG2Plan small = msm_plan_g2(1, 256, 2, MsmTuning{});
    std::printf("crossover=%zu sort_tile=%zu\n", (size_t)MSM_G2_CROSSOVER, small.chain.per_block);
    std::printf("all checks passed (%zu sizes)\n", ns.size());
    return 0;
}
