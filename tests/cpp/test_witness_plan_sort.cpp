// The witness-plan parser on blobs the Python side wrote (tests/test_witness_plan_sort_cpp.py): plans with SORT and ARGSORT records it must
// take, and plans with one defect each that it must refuse.  wplan_harness.hpp says what every blob goes through; here: what the sort
// kernels index with -- whole segments, a mode of 0 or 1, every source and destination a cell.
#include "wplan_harness.hpp"

int main(int argc, char** argv) {
    static_assert(SORT == 21 && ARGSORT == 22 && SORT_TILE == 2048, "the kinds are appended");
    static_assert(KINDS_TOP == 32, "the first kind past them all");
    check_kind_names();
    CHECK(!known(23) && std::string(kind_name(23)) == "?", "23 stays unassigned");
    unsigned n_sorts = 0, n_long = 0;
    run_manifest(argc, argv, [&](const Good& g) {
        const Plan& plan = g.plan;
        const uint64_t n_all = (uint64_t)plan.n_advice << plan.k;
        for (const Rec& r : plan.recs) {
            if (r.kind != SORT && r.kind != ARGSORT) continue;
            n_sorts++;
            n_long += r.p0 > SORT_TILE;
            CHECK(r.p0 >= 1 && r.count % r.p0 == 0 && r.p1 <= 1 && r.count <= MAX_SORT_COUNT, "%s: a sort record of %u cells in segments of %u, mode %u", g.file.c_str(), r.count, r.p0, r.p1);
            for (uint32_t e = 0; e < r.count; e++)
                CHECK(plan.pool[r.a + e] < n_all && plan.pool[r.dst + e] < n_all, "%s: element %u of a sort record is no cell", g.file.c_str(), e);
        }
    });
    CHECK(n_ok >= 6 && n_bad >= 15 && n_sorts >= 12 && n_long >= 2, "the manifest is thin: %u good, %u bad, %u sort records, %u above the tile", n_ok, n_bad, n_sorts, n_long);
    return finish();
}
