// The witness-plan parser (ezkl_amd/csrc/witness_plan.hpp) on blobs the Python side wrote: plans with the scan, gather and clamp kinds it
// must take, and plans with one defect each that it must refuse with the words the Python validator used.  A plain program: built with
// -fsanitize=address,undefined by tests/test_witness_plan_ops_cpp.py, so every index the parser forms from a blob's words is checked.
//
//   test_witness_plan_ops <dir>     <dir>/manifest.txt: one line per blob, "<file> <ok|bad> <the message expected, to the end of the line>"
//
// Every blob is also parsed cut short at every header boundary and a few places past it, and with each record's kind set to the first
// unknown one: the parser must refuse, not read past the buffer.
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
    const std::string dir = argv[1];
    std::ifstream manifest(dir + "/manifest.txt");
    std::string line;
    unsigned n_ok = 0, n_bad = 0, n_new_kinds = 0;
    while (std::getline(manifest, line)) {
        std::istringstream is(line);
        std::string file, verdict, want;
        is >> file >> verdict;
        std::getline(is, want);
        if (!want.empty() && want[0] == ' ') want.erase(0, 1);
        const std::vector<uint8_t> blob = slurp(dir + "/" + file);
        CHECK(!blob.empty(), "%s is empty or missing", file.c_str());
        Plan plan;
        std::string why;
        const bool ok = parse_exact(blob, blob.size(), plan, why);
        if (verdict == "ok") {
            n_ok++;
            CHECK(ok, "%s refused: %s", file.c_str(), why.c_str());
            if (!ok) continue;
            uint64_t cells = 0;
            for (const Rec& r : plan.recs) {
                if (r.kind >= SUMACC) n_new_kinds++;
                const bool scan = r.kind == DOT || r.kind == RLC || r.kind == SUMACC || r.kind == PRODACC;
                for (uint64_t i = 0; i < (scan ? (uint64_t)r.count * r.p1 : r.count); i++) cells += plan.pool[r.dst + i] != NONE;
                if (r.kind == GATHER)                    // what the kernel indexes with: the list inside the pool, every entry a cell
                    for (uint32_t i = 0; i < r.p1; i++) CHECK(plan.pool[r.p0 + i] < ((uint64_t)plan.n_advice << plan.k), "%s: a gather table entry is no cell", file.c_str());
            }
            CHECK(cells == plan.n_cells, "%s: %llu destinations, the header says %u", file.c_str(), (unsigned long long)cells, plan.n_cells);
            for (size_t cut : {(size_t)0, (size_t)1, (size_t)79, (size_t)111, (size_t)112, blob.size() / 2, blob.size() - 1}) {
                Plan p2;
                CHECK(!parse_exact(blob, cut < blob.size() ? cut : blob.size() - 1, p2, why), "%s cut to %zu bytes was taken", file.c_str(), cut);
            }
            const size_t recs_at = 112 + 8 * plan.params.size() + plan.consts.size();
            for (size_t ri = 0; ri < plan.recs.size(); ri++)         // one record's kind unassigned, or past the last: refused by name
                for (const uint32_t kind : {(uint32_t)UNASSIGNED, (uint32_t)N_KINDS}) {
                    std::vector<uint8_t> b2 = blob;
                    memcpy(b2.data() + recs_at + 32 * ri, &kind, 4);
                    Plan p2;
                    CHECK(!parse_exact(b2, b2.size(), p2, why) && why.find("unknown kind") != std::string::npos, "%s record %zu: %s", file.c_str(), ri, why.c_str());
                }
        } else {
            n_bad++;
            CHECK(!ok, "%s was taken, expected: %s", file.c_str(), want.c_str());
            CHECK(why == want, "%s: \"%s\", expected \"%s\"", file.c_str(), why.c_str(), want.c_str());
        }
    }
    CHECK(n_ok >= 4 && n_bad >= 10 && n_new_kinds >= 8, "the manifest is thin: %u good, %u bad, %u records of the new kinds", n_ok, n_bad, n_new_kinds);
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("%u good and %u bad blobs: all checks passed\n", n_ok, n_bad);
    return 0;
}
