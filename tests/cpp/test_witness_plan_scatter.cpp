// The witness-plan parser on blobs the Python side wrote (tests/test_witness_plan_scatter_cpp.py): plans with SCATTER, COMPLEMENT and ONEHOT
// records it must take, and plans with one defect each that it must refuse.  wplan_harness.hpp says what every blob goes through; here every
// word of every record of the three kinds, and every pool word of a SCATTER record's parameter array, is also set to a list of edge values:
// whatever the parser then answers, a plan it takes must satisfy what the kernels index with -- at least one element, a multiplier and an
// extent of at least 1, every target of an index inside the extent a destination, at most 2^28 cells, every base, index, source and
// destination a cell inside the pool's span; a complement of n - m cells over m <= n <= 2^28 sources; at least one one-hot class.
#include "wplan_harness.hpp"

static bool is_new(uint32_t kind) { return kind == SCATTER || kind == COMPLEMENT || kind == ONEHOT; }

// what the kernels of the three kinds index with, on a plan the parser took -> the number of records of the three kinds
static unsigned check_indexed(const Plan& plan, const char* file) {
    const uint64_t n_all = (uint64_t)plan.n_advice << plan.k, words = plan.pool.size();
    auto span = [&](uint32_t off, uint64_t n) { return off <= words && n <= words - off; };
    unsigned n = 0;
    for (const Rec& r : plan.recs) {
        if (!is_new(r.kind)) continue;
        n++;
        if (r.kind == SCATTER) {
            CHECK(r.p0 >= 1 && r.p1 >= 1 && r.count >= 1 && r.count <= MAX_SORT_COUNT, "%s: a scatter of %u elements at multiplier %u onto %u cells", file, r.p0, r.p1, r.count);
            CHECK(span(r.dst, r.count) && span(r.a, r.count) && span(r.b, 1 + 3ull * r.p0), "%s: a scatter record runs past the pool", file);
            if (!(r.p0 >= 1 && span(r.dst, r.count) && span(r.a, r.count) && span(r.b, 1 + 3ull * r.p0))) continue;
            const uint32_t extent = plan.pool[r.b];
            CHECK(extent >= 1, "%s: a scatter over an empty dimension", file);
            for (uint32_t j = 0; j < r.p0 && extent; j++) {
                CHECK(plan.pool[r.b + 1 + j] < n_all && plan.pool[r.b + 1 + r.p0 + j] < n_all, "%s: element %u of a scatter reads no cell", file, j);
                CHECK((uint64_t)plan.pool[r.b + 1 + 2ull * r.p0 + j] + (uint64_t)(extent - 1) * r.p1 < r.count, "%s: element %u of a scatter can leave its tensor", file, j);
            }
            for (uint32_t i = 0; i < r.count; i++) CHECK(plan.pool[r.dst + i] < n_all && plan.pool[r.a + i] < n_all, "%s: cell %u of a scatter is no cell", file, i);
        } else if (r.kind == COMPLEMENT) {
            CHECK(r.p1 <= r.p0 && r.count == r.p0 - r.p1 && r.p0 <= MAX_SORT_COUNT, "%s: a complement of %u cells over %u sources in a set of %u", file, r.count, r.p1, r.p0);
            CHECK(span(r.dst, r.count) && span(r.a, r.p1), "%s: a complement record runs past the pool", file);
            if (!(span(r.dst, r.count) && span(r.a, r.p1))) continue;
            for (uint32_t j = 0; j < r.p1; j++) CHECK(plan.pool[r.a + j] < n_all, "%s: source %u of a complement is no cell", file, j);
            for (uint32_t i = 0; i < r.count; i++) CHECK(plan.pool[r.dst + i] < n_all, "%s: destination %u of a complement is no cell", file, i);
        } else {
            CHECK(r.p0 >= 1 && r.count >= 1 && span(r.dst, r.count) && span(r.a, r.count) && span(r.b, r.count), "%s: a one-hot record of %u lanes over %u classes", file, r.count, r.p0);
            if (!(span(r.dst, r.count) && span(r.a, r.count))) continue;
            for (uint32_t i = 0; i < r.count; i++) CHECK(plan.pool[r.dst + i] < n_all && plan.pool[r.a + i] < n_all, "%s: lane %u of a one-hot record is no cell", file, i);
        }
    }
    return n;
}

int main(int argc, char** argv) {
    static_assert(DIVC == 15 && ARGSORT == 22 && RECIP == 24 && ISQRT == 25 && ARGEXT == 27 && SCATTER == 29 && COMPLEMENT == 30 && ONEHOT == 31 && KINDS_TOP == 32,
                  "16, 23, 26 and 28 stay unassigned; the kinds are appended after them");
    static_assert(VERSION == 1 && SORT_TILE == 2048 && ARGEXT_CHUNK == 4096 && SCATTER_TILE == 4096, "the pinned constants");
    check_kind_names();
    CHECK(!known(16) && !known(23) && !known(26) && !known(28) && !known(KINDS_TOP), "the unassigned kinds");
    unsigned n_claims = 0;
    run_manifest(argc, argv, [&](const Good& g) {
        const Plan& plan = g.plan;
        n_claims += check_indexed(plan, g.file.c_str());
        const uint32_t words = (uint32_t)plan.pool.size();
        auto on_taken = [&](const Plan& p2) { check_indexed(p2, g.file.c_str()); };
        for (size_t ri = 0; ri < plan.recs.size(); ri++) {
            const Rec& r = plan.recs[ri];
            if (!is_new(r.kind) || plan.pool.size() > 4096) continue;            // (the large plans: parsed, cut and renamed only)
            tamper_words(g.blob, g.recs_at, ri,
                         {0u, 1u, 2u, 3u, 5u, 6u, 7u, 64u, 4096u, 4097u, 1u << 28, (1u << 28) + 1, 0x55555555u, 0x55555556u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu, words - 1, words,
                          words + 1, r.count, r.p0},
                         on_taken);
            if (r.kind != SCATTER) continue;
            for (uint32_t w = 0; w < 1 + 3 * r.p0; w++)           // the extent, the index cells, the source cells, the offsets
                for (const uint32_t v : {0u, 1u, r.count - 1, r.count, r.count + 1, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu, (uint32_t)((uint64_t)plan.n_advice << plan.k)})
                    tamper(g.blob, g.pool_at + 4 * (r.b + w), v, on_taken);
        }
    });
    CHECK(n_ok >= 8 && n_bad >= 30 && n_claims >= 20 && n_tampered >= 1000 && n_taken >= 8 && n_taken < n_tampered,
          "the manifest is thin: %u good, %u bad, %u records of the new kinds, %u tampered words of which %u taken", n_ok, n_bad, n_claims, n_tampered, n_taken);
    return finish("words");
}
