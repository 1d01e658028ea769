// The witness-plan parser on version-2 blobs the Python side wrote (tests/test_contract_cpu.py): plans with CONTRACT records it must take,
// plans with one defect each that it must refuse with the Python validator's words, and every good blob again under a version-1 header:
// refused as an unknown kind.  (The manifest loop is this program's own: wplan_harness.hpp's sets kinds to 32 and expects "unknown".)
#include "wplan_harness.hpp"

int main(int argc, char** argv) {
    static_assert(VERSION == 1 && VERSION2 == 2 && KINDS_TOP == 32 && CONTRACT == 32 && KINDS2_TOP == 33, "the second table starts where the first ends");
    check_kind_names();
    CHECK(!known(CONTRACT) && known(CONTRACT, VERSION2) && !known(KINDS2_TOP, VERSION2) && std::string(kind_name(CONTRACT, VERSION2)) == "contract", "kind 32 by version");
    (void)check_truncations, (void)check_unknown_kinds;           // (the harness's own manifest loop is not this program's)
    if (argc != 2) return 2;
    const std::string dir = argv[1];
    std::ifstream manifest(dir + "/manifest.txt");
    std::string line;
    while (std::getline(manifest, line)) {
        std::istringstream is(line);
        std::string file, verdict, want, why;
        is >> file >> verdict;
        std::getline(is, want);
        if (!want.empty() && want[0] == ' ') want.erase(0, 1);
        std::vector<uint8_t> blob = slurp(dir + "/" + file);
        Plan plan, p1;
        const bool ok = !blob.empty() && parse_exact(blob, blob.size(), plan, why);
        if (verdict != "ok") {
            n_bad++;
            CHECK(!ok && why == want, "%s: \"%s\", expected \"%s\"", file.c_str(), why.c_str(), want.c_str());
            continue;
        }
        n_ok++;
        CHECK(ok && plan.version == VERSION2 && destinations(plan) == plan.n_cells, "%s: %s", file.c_str(), why.c_str());
        for (size_t cut : {(size_t)0, (size_t)111, blob.size() / 2, blob.size() - 4}) CHECK(!parse_exact(blob, cut, p1, why), "%s cut to %zu bytes was taken", file.c_str(), cut);
        blob[4] = 1;                                              // the same records under a version-1 header
        CHECK(!parse_exact(blob, blob.size(), p1, why) && why.find("(?): unknown kind") != std::string::npos, "%s as version 1: %s", file.c_str(), why.c_str());
    }
    CHECK(n_ok >= 2 && n_bad >= 5, "the manifest is thin: %u good, %u bad", n_ok, n_bad);
    return finish();
}
