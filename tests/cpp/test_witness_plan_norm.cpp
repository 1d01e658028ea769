// The witness-plan parser on blobs the Python side wrote (tests/test_witness_plan_norm_cpp.py): plans with RECIP and ISQRT records it must
// take, and plans with one defect each that it must refuse.  wplan_harness.hpp says what every blob goes through; here: what the two
// kernels index with -- a scale in [1, 2^62) and a zero-inverse index inside the constants for RECIP, a scale of at least 1 and no second
// parameter for ISQRT, every source and destination a cell.
#include "wplan_harness.hpp"

int main(int argc, char** argv) {
    static_assert(DIVC == 15 && ARGSORT == 22 && RECIP == 24 && ISQRT == 25, "16 and 23 stay unassigned; the kinds are appended after them");
    check_kind_names();
    CHECK(!known(16) && !known(23) && !known(26) && std::string(kind_name(16)) == "?" && std::string(kind_name(23)) == "?" && std::string(kind_name(26)) == "?", "the unassigned kinds");
    unsigned n_recips = 0, n_roots = 0;
    run_manifest(argc, argv, [&](const Good& g) {
        const Plan& plan = g.plan;
        const uint64_t n_all = (uint64_t)plan.n_advice << plan.k;
        for (const Rec& r : plan.recs) {
            if (r.kind != RECIP && r.kind != ISQRT) continue;
            if (r.kind == RECIP) {
                n_recips++;
                const uint64_t S = (uint64_t)r.p0 | ((uint64_t)r.p1 << 32);
                CHECK(S >= 1 && S < ((uint64_t)1 << 62) && r.b < plan.consts.size() / 32, "%s: a recip record at scale %llu with constant %u", g.file.c_str(),
                      (unsigned long long)S, r.b);
            } else {
                n_roots++;
                CHECK(r.p0 >= 1 && r.p1 == 0, "%s: a sqrt record at scale %u with a second parameter %u", g.file.c_str(), r.p0, r.p1);
            }
            for (uint32_t e = 0; e < r.count; e++)
                CHECK(plan.pool[r.a + e] < n_all && plan.pool[r.dst + e] < n_all, "%s: element %u of a %s record is no cell", g.file.c_str(), e, kind_name(r.kind));
        }
    });
    CHECK(n_ok >= 8 && n_bad >= 15 && n_recips >= 5 && n_roots >= 5, "the manifest is thin: %u good, %u bad, %u recip records, %u sqrt records", n_ok, n_bad, n_recips, n_roots);
    return finish();
}
