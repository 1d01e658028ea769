// What the test_witness_plan_*.cpp programs share.  Each is a plain program built with -fsanitize=address,undefined by tests/wplan_cpp.py, so
// every index the parser (ezkl_amd/csrc/witness_plan.hpp) forms from a blob's words is checked:
//
//   test_witness_plan_<family> <dir>     <dir>/manifest.txt: one line per blob, "<file> <ok|bad> <the message expected, to the end of the line>"
//
// A bad blob must be refused with the words the Python validator used.  A good blob must be taken, with as many destinations as its header
// says; it is then parsed cut short at every section boundary of its header and a few places past it, and with each record's kind set to
// every unassigned kind, to the first kind past them all and to 0xffffffff: the parser must refuse by name, not read past the buffer.  What
// the kernels of a family index with is that program's own checker, run on every plan the parser takes.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <fstream>
#include <initializer_list>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "witness_plan.hpp"

using namespace ezkl::wplan;

static int failures = 0;
static unsigned n_ok = 0, n_bad = 0, n_tampered = 0, n_taken = 0;
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

// a good blob as the parser took it, and where its sections begin
struct Good {
    std::string file;
    std::vector<uint8_t> blob;
    Plan plan;
    size_t recs_at, outs_at, pool_at;
};

// the destination words a plan names that are cells.  Which kinds are scans is stated here on purpose, not taken from the header's dst_words
static uint64_t destinations(const Plan& plan) {
    uint64_t cells = 0;
    for (const Rec& r : plan.recs) {
        const bool scan = r.kind == DOT || r.kind == RLC || r.kind == SUMACC || r.kind == PRODACC;
        for (uint64_t i = 0; i < (scan ? (uint64_t)r.count * r.p1 : r.count); i++) cells += plan.pool[r.dst + i] != NONE;
    }
    return cells;
}

static void check_truncations(const Good& g) {
    const size_t n = g.blob.size();
    std::string why;
    for (size_t cut : {(size_t)0, (size_t)1, (size_t)79, (size_t)111, (size_t)112, g.recs_at, g.recs_at + 31, g.outs_at, g.pool_at, g.pool_at + 4, n / 2, n - 4, n - 1}) {
        Plan p2;
        CHECK(!parse_exact(g.blob, cut < n ? cut : n - 1, p2, why), "%s cut to %zu bytes was taken", g.file.c_str(), cut);
    }
}

static void check_unknown_kinds(const Good& g) {
    std::string why;
    for (size_t ri = 0; ri < g.plan.recs.size(); ri++)
        for (const uint32_t kind : {16u, 23u, 26u, 28u, 32u, 0xFFFFFFFFu}) {
            std::vector<uint8_t> b2 = g.blob;
            memcpy(b2.data() + g.recs_at + 32 * ri, &kind, 4);
            Plan p2;
            CHECK(!parse_exact(b2, b2.size(), p2, why) && why.find("(?): unknown kind") != std::string::npos, "%s record %zu: %s", g.file.c_str(), ri, why.c_str());
        }
}

// one word of the blob replaced: whatever the parser answers it must not read past the buffer; taken -> on_taken(plan), refused -> by name
template <class OnTaken>
static void tamper(const std::vector<uint8_t>& blob, size_t at, uint32_t v, OnTaken on_taken) {
    std::vector<uint8_t> b2 = blob;
    memcpy(b2.data() + at, &v, 4);
    Plan p2;
    std::string why;
    n_tampered++;
    if (parse_exact(b2, b2.size(), p2, why)) {
        n_taken++;
        on_taken(p2);
    } else
        CHECK(why.rfind("witness plan: ", 0) == 0, "byte %zu = %u: \"%s\"", at, v, why.c_str());
}
// count, p0, p1, dst, a, b, phase of record ri: every word of the record at each of `values`
template <class OnTaken>
static void tamper_words(const std::vector<uint8_t>& blob, size_t recs_at, size_t ri, std::initializer_list<uint32_t> values, OnTaken on_taken) {
    for (int field = 1; field < 8; field++)
        for (const uint32_t v : values) tamper(blob, recs_at + 32 * ri + 4 * field, v, on_taken);
}

// the manifest of argv[1], blob by blob; on_good(g) after the checks every good blob gets
template <class OnGood>
static void run_manifest(int argc, char** argv, OnGood on_good) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <dir>\n", argv[0]);
        exit(2);
    }
    const std::string dir = argv[1];
    std::ifstream manifest(dir + "/manifest.txt");
    std::string line;
    while (std::getline(manifest, line)) {
        std::istringstream is(line);
        std::string verdict, want, why;
        Good g;
        is >> g.file >> verdict;
        std::getline(is, want);
        if (!want.empty() && want[0] == ' ') want.erase(0, 1);
        g.blob = slurp(dir + "/" + g.file);
        CHECK(!g.blob.empty(), "%s is empty or missing", g.file.c_str());
        if (g.blob.empty()) continue;
        const bool ok = parse_exact(g.blob, g.blob.size(), g.plan, why);
        if (verdict == "ok") {
            n_ok++;
            CHECK(ok, "%s refused: %s", g.file.c_str(), why.c_str());
            if (!ok) continue;
            const uint64_t cells = destinations(g.plan);
            CHECK(cells == g.plan.n_cells, "%s: %llu destinations, the header says %u", g.file.c_str(), (unsigned long long)cells, g.plan.n_cells);
            g.recs_at = 112 + 8 * g.plan.params.size() + g.plan.consts.size();
            g.outs_at = g.recs_at + 32 * g.plan.recs.size();
            g.pool_at = g.outs_at + 4 * g.plan.outputs.size();
            check_truncations(g);
            check_unknown_kinds(g);
            on_good(g);
        } else {
            n_bad++;
            CHECK(!ok, "%s was taken, expected: %s", g.file.c_str(), want.c_str());
            CHECK(why == want, "%s: \"%s\", expected \"%s\"", g.file.c_str(), why.c_str(), want.c_str());
        }
    }
}

// the names every kind number below KINDS_TOP has in a message, and "?" for anything else
static void check_kind_names() {
    static const char* const names[KINDS_TOP] = {"copy", "const", "input", "param", "add", "sub", "mult", "decompose", "range_check", "equals_zero", "dot",
                                                 "nonlinearity", "nonlinearity_index", "matmul", "rlc", "div", "?", "sum", "prod", "gather", "clamp", "sort",
                                                 "argsort", "?", "recip", "sqrt", "?", "argext", "?", "scatter", "complement", "one_hot"};
    for (uint32_t kind = 0; kind < KINDS_TOP; kind++) {
        CHECK(std::string(kind_name(kind)) == names[kind], "kind %u is named %s", kind, kind_name(kind));
        CHECK(known(kind) == (std::string(names[kind]) != "?"), "kind %u", kind);
    }
    for (const uint32_t kind : {(uint32_t)KINDS_TOP, 0xFFFFFFFFu}) CHECK(!known(kind) && std::string(kind_name(kind)) == "?", "kind %u", kind);
}

static int finish(const char* tampered_what = nullptr) {
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    if (tampered_what) printf("%u good and %u bad blobs, %u tampered %s: all checks passed\n", n_ok, n_bad, n_tampered, tampered_what);
    else printf("%u good and %u bad blobs: all checks passed\n", n_ok, n_bad);
    return 0;
}
