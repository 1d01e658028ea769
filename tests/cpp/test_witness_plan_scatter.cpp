// The witness-plan parser (ezkl_amd/csrc/witness_plan.hpp) on blobs the Python side wrote: plans with SCATTER, COMPLEMENT and ONEHOT records it
// must take, and plans with one defect each that it must refuse with the words the Python validator used.  A plain program: built with
// -fsanitize=address,undefined by tests/test_witness_plan_scatter_cpp.py, so every index the parser forms from a blob's words is checked.
//
//   test_witness_plan_scatter <dir>     <dir>/manifest.txt: one line per blob, "<file> <ok|bad> <the message expected, to the end of the line>"
//
// Every good blob is also parsed cut short at every section boundary of its header and a few places past it, with each record's kind set
// to the four unassigned ones (16, 23 = N_KINDS, 26 = KINDS_END, 28 = KINDS_LIMIT), to the end after the last kind and to 0xffffffff --
// refused by name -- and with every word of every record of a new kind, and every pool word of a SCATTER record's parameter array, set to a
// list of edge values: whatever the parser then answers, it must not read past the buffer, and a plan it takes must satisfy what the kernels
// index with -- at least one element, a multiplier and an extent of at least 1, every target of an index inside the extent a destination, at
// most 2^28 cells, every base, index, source and destination a cell inside the pool's span; a complement of n - m cells over m <= n <= 2^28
// sources; at least one one-hot class.
#include <stdio.h>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "witness_plan.hpp"

using namespace ezkl::wplan;

static int failures = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            failures++;                       \
            fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);     \
            fprintf(stderr, "\n");            \
        }                                     \
    } while (0)

static std::vector<uint8_t> slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

// the blob in a heap block of exactly its size: a read one byte past it is an AddressSanitizer report
static bool parse_exact(const std::vector<uint8_t>& blob, size_t len, Plan& plan, std::string& why) {
    std::vector<uint8_t> exact(blob.begin(), blob.begin() + len);
    exact.shrink_to_fit();
    return parse(len ? exact.data() : nullptr, len, plan, why);
}

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
    if (argc != 2) {
        fprintf(stderr, "usage: %s <dir>\n", argv[0]);
        return 2;
    }
    static_assert(UNASSIGNED == 16 && N_KINDS == 23 && RECIP == 24 && ISQRT == 25 && KINDS_END == 26 && ARGEXT == 27 && KINDS_LIMIT == 28 && SCATTER == 29 && COMPLEMENT == 30 &&
                      ONEHOT == 31 && KINDS_TOP == 32,
                  "16, 23, 26 and 28 stay unassigned; the kinds are appended after them");
    static_assert(VERSION == 1 && SORT_TILE == 2048 && ARGEXT_CHUNK == 4096 && SCATTER_TILE == 4096 && sizeof(KIND_NAMES) / sizeof(KIND_NAMES[0]) == 23, "the pinned constants");
    CHECK(std::string(kind_name(SCATTER)) == "scatter" && std::string(kind_name(COMPLEMENT)) == "complement" && std::string(kind_name(ONEHOT)) == "one_hot" &&
              std::string(kind_name(ARGEXT)) == "argext" && std::string(kind_name(COPY)) == "copy" && std::string(kind_name(UNASSIGNED)) == "?" &&
              std::string(kind_name(N_KINDS)) == "?" && std::string(kind_name(KINDS_END)) == "?" && std::string(kind_name(KINDS_LIMIT)) == "?" &&
              std::string(kind_name(KINDS_TOP)) == "?" && std::string(kind_name(0xFFFFFFFFu)) == "?",
          "kind names");
    const std::string dir = argv[1];
    std::ifstream manifest(dir + "/manifest.txt");
    std::string line;
    unsigned n_ok = 0, n_bad = 0, n_claims = 0, n_tampered = 0, n_taken = 0;
    while (std::getline(manifest, line)) {
        std::istringstream is(line);
        std::string file, verdict, want;
        is >> file >> verdict;
        std::getline(is, want);
        if (!want.empty() && want[0] == ' ') want.erase(0, 1);
        const std::vector<uint8_t> blob = slurp(dir + "/" + file);
        CHECK(!blob.empty(), "%s is empty or missing", file.c_str());
        if (blob.empty()) continue;
        Plan plan;
        std::string why;
        const bool ok = parse_exact(blob, blob.size(), plan, why);
        if (verdict == "ok") {
            n_ok++;
            CHECK(ok, "%s refused: %s", file.c_str(), why.c_str());
            if (!ok) continue;
            uint64_t cells = 0;
            for (const Rec& r : plan.recs) {
                const bool scan = r.kind == DOT || r.kind == RLC || r.kind == SUMACC || r.kind == PRODACC;
                for (uint64_t i = 0; i < (scan ? (uint64_t)r.count * r.p1 : r.count); i++) cells += plan.pool[r.dst + i] != NONE;
            }
            n_claims += check_indexed(plan, file.c_str());
            CHECK(cells == plan.n_cells, "%s: %llu destinations, the header says %u", file.c_str(), (unsigned long long)cells, plan.n_cells);
            const size_t recs_at = 112 + 8 * plan.params.size() + plan.consts.size(), outs_at = recs_at + 32 * plan.recs.size(), pool_at = outs_at + 4 * plan.outputs.size();
            for (size_t cut : {(size_t)0, (size_t)1, (size_t)79, (size_t)111, (size_t)112, recs_at, recs_at + 31, outs_at, pool_at, pool_at + 4, blob.size() / 2, blob.size() - 4,
                               blob.size() - 1}) {
                Plan p2;
                CHECK(!parse_exact(blob, cut < blob.size() ? cut : blob.size() - 1, p2, why), "%s cut to %zu bytes was taken", file.c_str(), cut);
            }
            const uint32_t words = (uint32_t)plan.pool.size();
            auto tamper = [&](size_t at, uint32_t v, const char* what, size_t ri, int field) {      // one word of the blob replaced: taken -> checked, refused -> by name
                std::vector<uint8_t> b2 = blob;
                memcpy(b2.data() + at, &v, 4);
                Plan p2;
                n_tampered++;
                if (parse_exact(b2, b2.size(), p2, why)) {
                    n_taken++;
                    check_indexed(p2, file.c_str());
                } else
                    CHECK(why.rfind("witness plan: ", 0) == 0, "%s record %zu %s %d = %u: \"%s\"", file.c_str(), ri, what, field, v, why.c_str());
            };
            for (size_t ri = 0; ri < plan.recs.size(); ri++) {
                for (const uint32_t kind : {(uint32_t)UNASSIGNED, (uint32_t)N_KINDS, (uint32_t)KINDS_END, (uint32_t)KINDS_LIMIT, (uint32_t)KINDS_TOP, 0xFFFFFFFFu}) {     // refused by name
                    std::vector<uint8_t> b2 = blob;
                    memcpy(b2.data() + recs_at + 32 * ri, &kind, 4);
                    Plan p2;
                    CHECK(!parse_exact(b2, b2.size(), p2, why) && why.find("(?): unknown kind") != std::string::npos, "%s record %zu: %s", file.c_str(), ri, why.c_str());
                }
                const Rec& r = plan.recs[ri];
                if (!is_new(r.kind) || plan.pool.size() > 4096) continue;            // (the large plans: parsed, cut and renamed only)
                for (int field = 1; field < 8; field++)              // count, p0, p1, dst, a, b, phase: every word of the record at its edges
                    for (const uint32_t v : {0u, 1u, 2u, 3u, 5u, 6u, 7u, 64u, 4096u, 4097u, 1u << 28, (1u << 28) + 1, 0x55555555u, 0x55555556u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu,
                                             0xFFFFFFFFu, words - 1, words, words + 1, r.count, r.p0})
                        tamper(recs_at + 32 * ri + 4 * field, v, "field", ri, field);
                if (r.kind != SCATTER) continue;
                for (uint32_t w = 0; w < 1 + 3 * r.p0; w++)           // the extent, the index cells, the source cells, the offsets
                    for (const uint32_t v : {0u, 1u, r.count - 1, r.count, r.count + 1, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu, (uint32_t)((uint64_t)plan.n_advice << plan.k)})
                        tamper(pool_at + 4 * (r.b + w), v, "pool word", ri, (int)w);
            }
        } else {
            n_bad++;
            CHECK(!ok, "%s was taken, expected: %s", file.c_str(), want.c_str());
            CHECK(why == want, "%s: \"%s\", expected \"%s\"", file.c_str(), why.c_str(), want.c_str());
        }
    }
    CHECK(n_ok >= 8 && n_bad >= 30 && n_claims >= 20 && n_tampered >= 1000 && n_taken >= 8 && n_taken < n_tampered,
          "the manifest is thin: %u good, %u bad, %u records of the new kinds, %u tampered words of which %u taken", n_ok, n_bad, n_claims, n_tampered, n_taken);
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("%u good and %u bad blobs, %u tampered words: all checks passed\n", n_ok, n_bad, n_tampered);
    return 0;
}
