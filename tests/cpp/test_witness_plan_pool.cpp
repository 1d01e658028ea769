// The witness-plan parser on blobs the Python side wrote (tests/test_witness_plan_pool_cpp.py): plans with ARGEXT records it must take, and
// plans with one defect each that it must refuse.  wplan_harness.hpp says what every blob goes through; here every word of every ARGEXT
// record is also set to a list of edge values: whatever the parser then answers, a plan it takes must satisfy what the kernels index with --
// a segment length of at least 1, a mode of 0 or 1, at most 2^28 sources, every source and destination a cell inside the pool's span.
#include "wplan_harness.hpp"

// what the arg-extremum kernels index with, on a plan the parser took -> the number of ARGEXT records
static unsigned check_argext(const Plan& plan, const char* file) {
    const uint64_t n_all = (uint64_t)plan.n_advice << plan.k;
    unsigned n = 0;
    for (const Rec& r : plan.recs) {
        if (r.kind != ARGEXT) continue;
        n++;
        const uint64_t sources = (uint64_t)r.count * r.p0;
        CHECK(r.p0 >= 1 && r.p1 <= 1 && r.count >= 1 && sources <= MAX_SORT_COUNT, "%s: an argext record of %u segments of %u in mode %u", file, r.count, r.p0, r.p1);
        CHECK(r.dst <= plan.pool.size() && r.count <= plan.pool.size() - r.dst && r.a <= plan.pool.size() && sources <= plan.pool.size() - r.a,
              "%s: an argext record runs past the pool", file);
        if (r.p0 < 1 || sources > plan.pool.size() || r.a > plan.pool.size() - sources || r.dst > plan.pool.size() - r.count) continue;
        for (uint64_t e = 0; e < sources; e++) CHECK(plan.pool[r.a + e] < n_all, "%s: source %llu of an argext record is no cell", file, (unsigned long long)e);
        for (uint32_t s = 0; s < r.count; s++) CHECK(plan.pool[r.dst + s] < n_all, "%s: destination %u of an argext record is no cell", file, s);
    }
    return n;
}

int main(int argc, char** argv) {
    static_assert(DIVC == 15 && ARGSORT == 22 && RECIP == 24 && ISQRT == 25 && ARGEXT == 27, "16, 23 and 26 stay unassigned; the kinds are appended after them");
    static_assert(VERSION == 1 && SORT_TILE == 2048 && ARGEXT_CHUNK == 4096 && KINDS_TOP == 32, "the pinned constants");
    check_kind_names();
    CHECK(!known(16) && !known(23) && !known(26) && !known(28) && std::string(kind_name(28)) == "?", "the unassigned kinds");
    unsigned n_claims = 0;
    run_manifest(argc, argv, [&](const Good& g) {
        const Plan& plan = g.plan;
        n_claims += check_argext(plan, g.file.c_str());
        const uint32_t words = (uint32_t)plan.pool.size();
        for (size_t ri = 0; ri < plan.recs.size(); ri++)
            if (plan.recs[ri].kind == ARGEXT)
                tamper_words(g.blob, g.recs_at, ri,
                             {0u, 1u, 2u, 3u, 64u, 65u, 4096u, 4097u, (1u << 26) + 1, (1u << 27) + 1, 1u << 28, (1u << 28) + 1, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu, words - 1,
                              words, words + 1, plan.recs[ri].count * plan.recs[ri].p0},
                             [&](const Plan& p2) { check_argext(p2, g.file.c_str()); });
    });
    CHECK(n_ok >= 8 && n_bad >= 15 && n_claims >= 8 && n_tampered >= 1000 && n_taken >= 8 && n_taken < n_tampered,
          "the manifest is thin: %u good, %u bad, %u argext records, %u tampered words of which %u taken", n_ok, n_bad, n_claims, n_tampered, n_taken);
    return finish("records");
}
