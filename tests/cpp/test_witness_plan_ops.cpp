// The witness-plan parser on blobs the Python side wrote (tests/test_witness_plan_ops_cpp.py): plans with the scan, gather and clamp kinds it
// must take, and plans with one defect each that it must refuse.  wplan_harness.hpp says what every blob goes through; here: a gather
// table is a list inside the pool, every entry a cell.
#include "wplan_harness.hpp"

int main(int argc, char** argv) {
    static_assert(SUMACC == 17 && PRODACC == 18 && GATHER == 19 && CLAMP == 20, "the kinds are appended");
    check_kind_names();
    unsigned n_new_kinds = 0;
    run_manifest(argc, argv, [&](const Good& g) {
        for (const Rec& r : g.plan.recs) {
            if (r.kind >= SUMACC) n_new_kinds++;
            if (r.kind == GATHER)                    // what the kernel indexes with: the list inside the pool, every entry a cell
                for (uint32_t i = 0; i < r.p1; i++)
                    CHECK(g.plan.pool[r.p0 + i] < ((uint64_t)g.plan.n_advice << g.plan.k), "%s: a gather table entry is no cell", g.file.c_str());
        }
    });
    CHECK(n_ok >= 4 && n_bad >= 10 && n_new_kinds >= 8, "the manifest is thin: %u good, %u bad, %u records of the new kinds", n_ok, n_bad, n_new_kinds);
    return finish();
}
