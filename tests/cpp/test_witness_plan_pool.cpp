// The witness-plan parser (ezkl_amd/csrc/witness_plan.hpp) on blobs the Python side wrote: plans with ARGEXT records it must take, and
// plans with one defect each that it must refuse with the words the Python validator used.  A plain program: built with
// -fsanitize=address,undefined by tests/test_witness_plan_pool_cpp.py, so every index the parser forms from a blob's words is checked.
//
//   test_witness_plan_pool <dir>     <dir>/manifest.txt: one line per blob, "<file> <ok|bad> <the message expected, to the end of the line>"
//
// Every good blob is also parsed cut short at every section boundary of its header and a few places past it, with each record's kind set
// to the three unassigned ones (16, 23 = N_KINDS, 26 = KINDS_END), to the limit after the last kind and to 0xffffffff -- refused by name --
// and with every word of every ARGEXT record set to a list of edge values: whatever the parser then answers, it must not read past the
// buffer, and a plan it takes must satisfy what the kernels index with -- a segment length of at least 1, a mode of 0 or 1, at most 2^28
// sources, every source and destination a cell inside the pool's span, the destination count the header's n_cells.
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
    if (argc != 2) {
        fprintf(stderr, "usage: %s <dir>\n", argv[0]);
        return 2;
    }
    static_assert(UNASSIGNED == 16 && N_KINDS == 23 && RECIP == 24 && ISQRT == 25 && KINDS_END == 26 && ARGEXT == 27 && KINDS_LIMIT == 28,
                  "16, 23 and 26 stay unassigned; the kinds are appended after them");
    static_assert(VERSION == 1 && SORT_TILE == 2048 && ARGEXT_CHUNK == 4096 && sizeof(KIND_NAMES) / sizeof(KIND_NAMES[0]) == 23, "the pinned constants");
    CHECK(std::string(kind_name(ARGEXT)) == "argext" && std::string(kind_name(ISQRT)) == "sqrt" && std::string(kind_name(ARGSORT)) == "argsort" &&
              std::string(kind_name(COPY)) == "copy" && std::string(kind_name(UNASSIGNED)) == "?" && std::string(kind_name(N_KINDS)) == "?" &&
              std::string(kind_name(KINDS_END)) == "?" && std::string(kind_name(KINDS_LIMIT)) == "?" && std::string(kind_name(0xFFFFFFFFu)) == "?",
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
            n_claims += check_argext(plan, file.c_str());
            CHECK(cells == plan.n_cells, "%s: %llu destinations, the header says %u", file.c_str(), (unsigned long long)cells, plan.n_cells);
            const size_t recs_at = 112 + 8 * plan.params.size() + plan.consts.size(), outs_at = recs_at + 32 * plan.recs.size(), pool_at = outs_at + 4 * plan.outputs.size();
            for (size_t cut : {(size_t)0, (size_t)1, (size_t)79, (size_t)111, (size_t)112, recs_at, recs_at + 31, outs_at, pool_at, pool_at + 4, blob.size() / 2, blob.size() - 4,
                               blob.size() - 1}) {
                Plan p2;
                CHECK(!parse_exact(blob, cut < blob.size() ? cut : blob.size() - 1, p2, why), "%s cut to %zu bytes was taken", file.c_str(), cut);
            }
            for (size_t ri = 0; ri < plan.recs.size(); ri++) {
                for (const uint32_t kind : {(uint32_t)UNASSIGNED, (uint32_t)N_KINDS, (uint32_t)KINDS_END, (uint32_t)KINDS_LIMIT, 0xFFFFFFFFu}) {     // refused by name
                    std::vector<uint8_t> b2 = blob;
                    memcpy(b2.data() + recs_at + 32 * ri, &kind, 4);
                    Plan p2;
                    CHECK(!parse_exact(b2, b2.size(), p2, why) && why.find("(?): unknown kind") != std::string::npos, "%s record %zu: %s", file.c_str(), ri, why.c_str());
                }
                if (plan.recs[ri].kind != ARGEXT) continue;
                const uint32_t words = (uint32_t)plan.pool.size();
                for (int field = 1; field < 8; field++)              // count, p0, p1, dst, a, b, phase: every word of the record at its edges
                    for (const uint32_t v : {0u, 1u, 2u, 3u, 64u, 65u, 4096u, 4097u, (1u << 26) + 1, (1u << 27) + 1, 1u << 28, (1u << 28) + 1, 0x7FFFFFFFu, 0x80000000u,
                                             0xFFFFFFFEu, 0xFFFFFFFFu, words - 1, words, words + 1, plan.recs[ri].count * plan.recs[ri].p0}) {
                        std::vector<uint8_t> b2 = blob;
                        memcpy(b2.data() + recs_at + 32 * ri + 4 * field, &v, 4);
                        Plan p2;
                        n_tampered++;
                        if (parse_exact(b2, b2.size(), p2, why)) {
                            n_taken++;
                            check_argext(p2, file.c_str());
                        } else
                            CHECK(why.rfind("witness plan: ", 0) == 0, "%s record %zu field %d = %u: \"%s\"", file.c_str(), ri, field, v, why.c_str());
                    }
            }
        } else {
            n_bad++;
            CHECK(!ok, "%s was taken, expected: %s", file.c_str(), want.c_str());
            CHECK(why == want, "%s: \"%s\", expected \"%s\"", file.c_str(), why.c_str(), want.c_str());
        }
    }
    CHECK(n_ok >= 8 && n_bad >= 15 && n_claims >= 8 && n_tampered >= 1000 && n_taken >= 8 && n_taken < n_tampered,
          "the manifest is thin: %u good, %u bad, %u argext records, %u tampered words of which %u taken", n_ok, n_bad, n_claims, n_tampered, n_taken);
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("%u good and %u bad blobs, %u tampered records: all checks passed\n", n_ok, n_bad, n_tampered);
    return 0;
}
