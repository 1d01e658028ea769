// The plan of an MSM without window tables (ezkl_amd/csrc/msm_plan.hpp: pick_plan_once and msm_plan_once) held to what msm_once_run and the
// kernels it launches rely on, and the identity the path computes by -- recode, one sum per window, combine -- restated on integers.  A
// stand-alone program, built by tests/test_msm_once_plan_cpp.py under AddressSanitizer and UndefinedBehaviorSanitizer.  No device.
//
// Sweep: every n in 1 .. 4096; 2^k - 1, 2^k, 2^k + 1 for k = 13 .. 26; 1000 random n below 2^26; devices of 1, 8, 64, 256 and 304 CUs with
// 1, 2 or 3 resident accumulate workgroups per CU; the default tuning and L_override 8 / 64.  For every plan:
//   windows   W >= 12, the widths sum to 254 (>= the 254 bits of a folded scalar and its last carry), differ by at most one, the wider
//             ones first; 2 <= width <= cmax <= 23 (msm_recode's bit buffer); msm_plan_once carries pick_plan_once's plan
//   groups    1 <= group <= MSM_MAX_GROUP; ngroups groups of `group` windows cover W and none is empty; a group's slabs stay inside
//             MSM_ONCE_SCRATCH_CAP unless the group is a single window
//   chain     ONE window: W == 1, bits == cmax - 1, so every bucket id of every window (< 2^(width - 1)) is below nb; sized for n pairs;
//             tiles of 64 .. 1024 scalars whose pairs (one per scalar at the most) fit the partition kernel's stage inside MSM_PART_LDS; the
//             histogram's LDS row holds NQ counts; lanes cover n pairs; at most 32 planes per window (the landing buffer's record block);
//             bstride == slab_bytes for a group of several windows, 0 for one
//   scratch   the converted points [o_points, + 64 n) and the `group` slabs [o_slabs + z * slab_bytes, + slab_bytes) are pairwise disjoint,
//             256-byte aligned and end inside `bytes`; every region of a slab starts inside it, and the pair / payload / bucket / lane regions
//             are as large as the launches are told (the layout inside a slab is msm_plan's: tests/cpp/test_msm_plan.cpp)
//   payload   n < 2^31: an index and the sign bit
// and the plans of 2^16 and 2^20 points on a 256-CU device are pinned.
// Identity: for edge scalars and 20 000 random ones under balanced plans of 12 .. 127 windows, the signed digits d_w of the recoding -- the
// algorithm of msm.hip's msm_recode: eight 32-bit limbs into a 64-bit buffer, raw > half -> raw - 2^c and a carry -- satisfy
// sum_w 2^offset(w) d_w == s for s <= (r - 1) / 2 and == -(r - s) beyond (the fold, signs flipped), with the sum taken as the host tail takes
// it: acc = d_{W-1}, then acc = 2^width(w) acc + d_w for w = W-2 .. 0.  Also: the buffer never holds more than 54 bits before a refill, every
// window is emitted by the time the eighth limb is in, the last carry is zero and |d_w| <= 2^(width(w) - 1).
#include "msm_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

using namespace ezkl;

static size_t g_checks = 0;
struct Case {
    size_t n;
    int num_cus, occ;
    uint32_t L_override;
};
[[noreturn]] static void fail(const Case& c, const char* what) {
    printf("FAILED: %s\n  at n=%zu num_cus=%d acc_blocks_per_cu=%d L_override=%u\n", what, c.n, c.num_cus, c.occ, c.L_override);
    exit(1);
}
#define CHECK(cond) do { g_checks++; if (!(cond)) fail(c, #cond); } while (0)

static void check_windows(const Case& c, const WinPlan& wp) {
    CHECK(wp.W >= 12 && wp.W <= 127);
    uint32_t sum = 0, lo = 99, hi = 0;
    bool ordered = true;
    for (uint32_t w = 0; w < wp.W; w++) {
        const uint32_t c_w = wp.width(w);
        CHECK(wp.offset(w) == sum);
        sum += c_w;
        lo = c_w < lo ? c_w : lo;
        hi = c_w > hi ? c_w : hi;
        if (w && c_w > wp.width(w - 1)) ordered = false;
    }
    CHECK(sum == 254 && wp.offset(wp.W) == 254);
    CHECK(hi - lo <= 1 && ordered);
    CHECK(lo >= 2 && hi == wp.cmax() && wp.cmax() <= 23);
}

static void check(const Case& c) {
    MsmTuning tu;
    tu.L_override = c.L_override;
    const MsmOncePlan q = msm_plan_once(c.n, c.num_cus, c.occ, tu);
    const WinPlan wp = pick_plan_once(c.n);
    CHECK(q.wp.W == wp.W && q.wp.base == wp.base && q.wp.rem == wp.rem);
    check_windows(c, wp);
    // groups
    CHECK(q.group >= 1 && q.group <= MSM_MAX_GROUP && q.ngroups >= 1);
    CHECK(q.ngroups * q.group >= wp.W && (q.ngroups - 1) * q.group < wp.W);
    const MsmPlan& p = q.chain;
    CHECK(q.group * p.slab_bytes <= MSM_ONCE_SCRATCH_CAP || q.group == 1);
    // one window's chain
    CHECK(p.W == 1 && p.bits == wp.cmax() - 1 && p.nb == 1u << p.bits && p.npairs == c.n);
    for (uint32_t w = 0; w < wp.W; w++) CHECK(((uint32_t)1 << (wp.width(w) - 1)) <= p.nb);
    CHECK(p.per_block % 64 == 0 && p.per_block >= 64 && p.per_block <= 1024);
    CHECK(p.part_lds == (3 * ((size_t)p.NQ + 1) + 2 * p.per_block) * 4 && p.part_lds <= MSM_PART_LDS);
    CHECK(p.NQ == p.NP + 1 && p.NQ <= (1u << MSM_MAX_PART_BITS) + 1);
    CHECK((size_t)MSM_BINSORT_STAGE * 4 <= MSM_BINSORT_LDS);
    CHECK((size_t)p.sgrid * p.per_block >= c.n && c.n > ((size_t)p.sgrid - 1) * p.per_block);
    CHECK(p.L >= 8 && (size_t)p.nlanes * p.L >= c.n && c.n > ((size_t)p.nlanes - 1) * p.L);
    CHECK(c.L_override == 0 || p.L == c.L_override);
    CHECK(p.nplanes == 1 + p.bits && p.nplanes <= 32);
    CHECK(p.bstride == (q.group > 1 ? p.slab_bytes : 0));
    CHECK(p.zero_bytes % 4 == 0 && p.zero_bytes / 4 <= 0xffffffffu);
    // scratch
    CHECK(q.o_points == 0 && q.o_points % 256 == 0 && q.o_slabs % 256 == 0 && p.slab_bytes % 256 == 0);
    CHECK(q.o_points + c.n * 64 <= q.o_slabs);
    CHECK(q.bytes == q.o_slabs + q.group * p.slab_bytes);
    const size_t PT = MSM_POINT_BYTES;
    const size_t offs[] = {p.o.ent, p.o.vals, p.o.offs, p.o.pcnt, p.o.pbase, p.o.wghist, p.o.heavy, p.o.chunks, p.o.hcnt, p.o.btot, p.o.planes,
                           p.o.bflag, p.o.blist, p.o.boff, p.o.lfirst, p.o.bkt, p.o.head, p.o.tail, p.o.partA, p.o.partT, p.o.SA, p.o.T};
    for (size_t o : offs) CHECK(o % 256 == 0 && o < p.slab_bytes);
    CHECK(p.o.ent + c.n * 8 <= p.o.vals && p.o.vals + c.n * 4 <= p.o.offs && p.o.offs + ((size_t)p.nb + 1) * 4 <= p.o.pcnt);
    CHECK(p.o.wghist + (size_t)p.sgrid * p.NQ * 4 <= p.o.heavy);
    CHECK(p.o.lfirst + (size_t)p.nlanes * 4 <= p.o.bkt && p.o.bkt + (size_t)p.nb * PT <= p.o.head);
    CHECK(p.o.head + (size_t)p.nlanes * PT <= p.o.tail && p.o.tail + (size_t)p.nlanes * PT <= p.o.partA);
    CHECK(p.o.T + (size_t)p.nT * PT <= p.slab_bytes);
    // payload
    CHECK(c.n < ((size_t)1 << 31));
}

// ---- the identity on integers -------------------------------------------------------------------------------------------------------
// r = the order of BN254's G1, four 64-bit limbs
static const uint64_t RMOD[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
struct U256 { uint64_t v[4]; };
static int cmp(const U256& a, const U256& b) {
    for (int i = 3; i >= 0; i--)
        if (a.v[i] != b.v[i]) return a.v[i] < b.v[i] ? -1 : 1;
    return 0;
}
static U256 sub(const U256& a, const U256& b) {
    U256 r;
    unsigned __int128 br = 0;
    for (int i = 0; i < 4; i++) {
        const unsigned __int128 d = (unsigned __int128)a.v[i] - b.v[i] - br;
        r.v[i] = (uint64_t)d;
        br = (d >> 64) & 1;
    }
    return r;
}
// a signed integer of 320 bits, two's complement, for the Horner sums
struct S320 { uint64_t v[5]; };
static S320 from_small(int64_t x) {
    S320 r;
    r.v[0] = (uint64_t)x;
    for (int i = 1; i < 5; i++) r.v[i] = x < 0 ? ~(uint64_t)0 : 0;
    return r;
}
static S320 shl(const S320& a, uint32_t c) {                 // 0 < c < 64
    S320 r;
    for (int i = 4; i >= 0; i--) r.v[i] = (a.v[i] << c) | (i ? a.v[i - 1] >> (64 - c) : 0);
    return r;
}
static S320 add(const S320& a, const S320& b) {
    S320 r;
    unsigned __int128 cy = 0;
    for (int i = 0; i < 5; i++) {
        cy += (unsigned __int128)a.v[i] + b.v[i];
        r.v[i] = (uint64_t)cy;
        cy >>= 64;
    }
    return r;
}
static S320 neg(const S320& a) {
    S320 r;
    for (int i = 0; i < 5; i++) r.v[i] = ~a.v[i];
    return add(r, from_small(1));
}
static S320 from_u256(const U256& a) { return S320{{a.v[0], a.v[1], a.v[2], a.v[3], 0}}; }

static size_t g_scalars = 0;
// s: canonical (< r).  The digits as msm_canon + msm_recode make them, then the combine in the host tail's order.
static void identity(const WinPlan& wp, const U256& s) {
    const Case c{0, 0, 0, 0};
    U256 half_r;                                            // (r - 1) / 2
    for (int i = 0; i < 4; i++) half_r.v[i] = (RMOD[i] >> 1) | (i < 3 ? RMOD[i + 1] << 63 : 0);
    U256 rm;
    memcpy(rm.v, RMOD, sizeof RMOD);
    const bool negd = cmp(s, half_r) > 0;
    const U256 m = negd ? sub(rm, s) : s;
    uint32_t limb[8];
    for (int k = 0; k < 8; k++) limb[k] = (uint32_t)(m.v[k / 2] >> (32 * (k & 1)));
    std::vector<int64_t> d(wp.W, 0);
    uint64_t buf = 0;
    uint32_t carry = 0, have = 0, w = 0, cw = wp.width(0);
    for (int k = 0; k < 8; k++) {
        CHECK(have < cw || w >= wp.W);                      // before a refill fewer bits than a window: have + 32 <= 54
        CHECK(have + 32 <= 64);
        buf |= (uint64_t)limb[k] << have;
        have += 32;
        while (have >= cw && w < wp.W) {
            const uint32_t full = 1u << cw, half = full >> 1;
            const uint32_t raw = ((uint32_t)buf & (full - 1u)) + carry;
            buf >>= cw;
            const uint32_t minus = raw > half ? 1u : 0u;
            const uint32_t mag = minus ? full - raw : raw;
            carry = minus;
            CHECK(mag <= half);                             // bucket = mag - 1 < 2^(width - 1)
            d[w] = (minus ^ (negd ? 1u : 0u)) ? -(int64_t)mag : (int64_t)mag;
            have -= cw;
            w++;
            cw = wp.width(w);
        }
    }
    CHECK(w == wp.W && carry == 0 && buf == 0);
    S320 acc = from_small(d[wp.W - 1]);
    for (uint32_t x = wp.W - 1; x-- > 0;) acc = add(shl(acc, wp.width(x)), from_small(d[x]));
    const S320 want = negd ? neg(from_u256(m)) : from_u256(m);
    CHECK(memcmp(acc.v, want.v, sizeof acc.v) == 0);
    g_scalars++;
}

static void identities() {
    // the plans pick_plan_once chooses at 2^26, 2^24 and 2^20 points and below (12, 13, 16 windows) and balanced plans it could choose
    // under another cost model, up to the narrowest
    const uint32_t windows[] = {12, 13, 14, 15, 16, 22, 32, 64, 127};
    std::mt19937_64 rng(29);
    U256 rm, one{{1, 0, 0, 0}};
    memcpy(rm.v, RMOD, sizeof RMOD);
    U256 half_r;
    for (int i = 0; i < 4; i++) half_r.v[i] = (RMOD[i] >> 1) | (i < 3 ? RMOD[i + 1] << 63 : 0);
    for (uint32_t W : windows) {
        const WinPlan wp{W, 254 / W, 254 % W};
        check_windows(Case{0, 0, 0, W}, wp);
        std::vector<U256> ss = {U256{{0, 0, 0, 0}}, one, sub(rm, one), half_r, sub(rm, half_r) /* (r + 1) / 2 */, U256{{2, 0, 0, 0}}, sub(rm, U256{{2, 0, 0, 0}})};
        // every window 2^c - 1 (all ones below bit 253), every window 2^(c-1) + 1, and runs of one-bits of every length: carries through all
        // windows into the top one; values above (r - 1) / 2 come back through the fold
        U256 ones{{~(uint64_t)0, ~(uint64_t)0, ~(uint64_t)0, ((uint64_t)1 << 61) - 1}}, pat{{0, 0, 0, 0}};
        ss.push_back(ones);
        for (uint32_t w = 0; w < wp.W; w++) {
            const uint32_t o = wp.offset(w), cw = wp.width(w);
            for (uint32_t bit : {o, o + cw - 1})
                if (bit < 253) pat.v[bit / 64] |= (uint64_t)1 << (bit % 64);
        }
        ss.push_back(pat);
        for (uint32_t k = 1; k <= 253; k++) {
            U256 run{{0, 0, 0, 0}};
            for (uint32_t b = 0; b < k; b++) run.v[b / 64] |= (uint64_t)1 << (b % 64);
            ss.push_back(run);
            ss.push_back(sub(rm, run));
        }
        for (int i = 0; i < 20000; i++) {
            U256 s{{rng(), rng(), rng(), rng() & (((uint64_t)1 << 61) - 1)}};      // 253 bits: below r
            if (i % 4 == 1) s = U256{{rng() & 0xfffff, 0, 0, 0}};                   // witness-like: 20 bits, and its negative
            if (i % 4 == 2) s = sub(rm, U256{{1 + (rng() & 0xfffff), 0, 0, 0}});
            ss.push_back(s);
        }
        for (const U256& s : ss)
            if (cmp(s, rm) < 0) identity(wp, s);
    }
}

static void table() {
    const Case c{(size_t)1 << 20, 256, 3, 0};
    const MsmOncePlan q = msm_plan_once(c.n, 256, 3, MsmTuning());
    CHECK(q.wp.W == 16 && q.wp.base == 15 && q.wp.rem == 14 && q.group == 16 && q.ngroups == 1 && q.chain.bits == 15);       // 14 x 16 + 2 x 15 bits
    const MsmOncePlan s = msm_plan_once((size_t)1 << 16, 256, 3, MsmTuning());
    CHECK(s.wp.W == 16 && s.group == 16 && s.ngroups == 1);                            // a second sequence of launches costs more than wider windows
    const MsmOncePlan t = msm_plan_once(1, 256, 3, MsmTuning());
    CHECK(t.wp.W == 16 && t.ngroups == 1);
    const MsmOncePlan b = msm_plan_once((size_t)1 << 26, 256, 3, MsmTuning());
    CHECK(b.group * b.chain.slab_bytes <= MSM_ONCE_SCRATCH_CAP && b.ngroups > 1);      // the cap at work
}

int main() {
    std::vector<size_t> ns;
    for (size_t n = 1; n <= 4096; n++) ns.push_back(n);
    for (int k = 13; k <= 26; k++)
        for (int d = -1; d <= 1; d++) ns.push_back(((size_t)1 << k) + d);
    std::mt19937_64 rng(17);
    for (int i = 0; i < 1000; i++) ns.push_back(1 + rng() % ((size_t)1 << 26));
    const int cus[] = {1, 8, 64, 256, 304}, occ[] = {1, 2, 3};
    const uint32_t lov[] = {0, 8, 64};
    size_t plans = 0;
    table();
    for (size_t n : ns)
        for (int cu : cus)
            for (int o : occ)
                for (uint32_t l : lov) {
                    check(Case{n, cu, o, l});
                    plans++;
                }
    identities();
    printf("all checks passed: %zu sizes, %zu plans, %zu scalars, %zu checks\n", ns.size(), plans, g_scalars, g_checks);
    return 0;
}
