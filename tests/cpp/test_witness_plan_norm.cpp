// The witness-plan parser (ezkl_amd/csrc/witness_plan.hpp) on blobs the Python side wrote: plans with RECIP and ISQRT records it must take,
// and plans with one defect each that it must refuse with the words the Python validator used.  A plain program: built with
// -fsanitize=address,undefined by tests/test_witness_plan_norm_cpp.py, so every index the parser forms from a blob's words is checked.
//
//   test_witness_plan_norm <dir>     <dir>/manifest.txt: one line per blob, "<file> <ok|bad> <the message expected, to the end of the line>"
//
// Every good blob is also parsed cut short at every section boundary of its header and a few places past it, and with each record's
// kind set to the two unassigned ones (16 and 23 = N_KINDS), to the end marker after the last kind and to 0xffffffff: the parser must refuse
// by name, not read past the buffer.  What the two kernels index with is checked on the parsed plan: a scale in [1, 2^62) and a
// zero-inverse index inside the constants for RECIP, a scale of at least 1 and no second parameter for ISQRT, every source and destination
// a cell, the destination count the header's n_cells.
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

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <dir>\n", argv[0]);
        return 2;
    }
    static_assert(UNASSIGNED == 16 && N_KINDS == 23 && RECIP == 24 && ISQRT == 25 && KINDS_END == 26, "23 stays unassigned; the kinds are appended after it");
    CHECK(std::string(kind_name(RECIP)) == "recip" && std::string(kind_name(ISQRT)) == "sqrt" && std::string(kind_name(ARGSORT)) == "argsort" &&
              std::string(kind_name(COPY)) == "copy" && std::string(kind_name(UNASSIGNED)) == "?" && std::string(kind_name(N_KINDS)) == "?" &&
              std::string(kind_name(KINDS_END)) == "?" && std::string(kind_name(0xFFFFFFFFu)) == "?",
          "kind names");
    const std::string dir = argv[1];
    std::ifstream manifest(dir + "/manifest.txt");
    std::string line;
    unsigned n_ok = 0, n_bad = 0, n_recips = 0, n_roots = 0;
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
            const uint64_t n_all = (uint64_t)plan.n_advice << plan.k;
            uint64_t cells = 0;
            for (const Rec& r : plan.recs) {
                const bool scan = r.kind == DOT || r.kind == RLC || r.kind == SUMACC || r.kind == PRODACC;
                for (uint64_t i = 0; i < (scan ? (uint64_t)r.count * r.p1 : r.count); i++) cells += plan.pool[r.dst + i] != NONE;
                if (r.kind != RECIP && r.kind != ISQRT) continue;
                if (r.kind == RECIP) {
                    n_recips++;
                    const uint64_t S = (uint64_t)r.p0 | ((uint64_t)r.p1 << 32);
                    CHECK(S >= 1 && S < ((uint64_t)1 << 62) && r.b < plan.consts.size() / 32, "%s: a recip record at scale %llu with constant %u", file.c_str(),
                          (unsigned long long)S, r.b);
                } else {
                    n_roots++;
                    CHECK(r.p0 >= 1 && r.p1 == 0, "%s: a sqrt record at scale %u with a second parameter %u", file.c_str(), r.p0, r.p1);
                }
                for (uint32_t e = 0; e < r.count; e++)
                    CHECK(plan.pool[r.a + e] < n_all && plan.pool[r.dst + e] < n_all, "%s: element %u of a %s record is no cell", file.c_str(), e, kind_name(r.kind));
            }
            CHECK(cells == plan.n_cells, "%s: %llu destinations, the header says %u", file.c_str(), (unsigned long long)cells, plan.n_cells);
            const size_t recs_at = 112 + 8 * plan.params.size() + plan.consts.size(), outs_at = recs_at + 32 * plan.recs.size(), pool_at = outs_at + 4 * plan.outputs.size();
            for (size_t cut : {(size_t)0, (size_t)1, (size_t)79, (size_t)111, (size_t)112, recs_at, recs_at + 31, outs_at, pool_at, pool_at + 4, blob.size() / 2, blob.size() - 4,
                               blob.size() - 1}) {
                Plan p2;
                CHECK(!parse_exact(blob, cut < blob.size() ? cut : blob.size() - 1, p2, why), "%s cut to %zu bytes was taken", file.c_str(), cut);
            }
            for (size_t ri = 0; ri < plan.recs.size(); ri++)         // one record's kind unassigned, or past the last: refused by name
                for (const uint32_t kind : {(uint32_t)UNASSIGNED, (uint32_t)N_KINDS, (uint32_t)KINDS_END, 0xFFFFFFFFu}) {
                    std::vector<uint8_t> b2 = blob;
                    memcpy(b2.data() + recs_at + 32 * ri, &kind, 4);
                    Plan p2;
                    CHECK(!parse_exact(b2, b2.size(), p2, why) && why.find("(?): unknown kind") != std::string::npos, "%s record %zu: %s", file.c_str(), ri, why.c_str());
                }
        } else {
            n_bad++;
            CHECK(!ok, "%s was taken, expected: %s", file.c_str(), want.c_str());
            CHECK(why == want, "%s: \"%s\", expected \"%s\"", file.c_str(), why.c_str(), want.c_str());
        }
    }
    CHECK(n_ok >= 8 && n_bad >= 15 && n_recips >= 5 && n_roots >= 5, "the manifest is thin: %u good, %u bad, %u recip records, %u sqrt records", n_ok, n_bad, n_recips, n_roots);
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("%u good and %u bad blobs: all checks passed\n", n_ok, n_bad);
    return 0;
}
