// The point predicate of ezkl_amd/csrc/srs_check.hpp as a plain program (no device, no HIP headers), built by tests/test_srs_check_cpp.py
// under AddressSanitizer and UndefinedBehaviorSanitizer.
//
//   test_srs_check <cases>     cases: records of 65 bytes -- the 64-byte point record, then what tests/srs_check_ref.py says of it:
//                              reason | identity << 2
// Every record goes through point_reason<FqPortable>; the first disagreement is printed with its index and the program fails.  Before
// the file it holds the portable field to two identities the predicate leans on: one * one == one (R * R / R) and 3 == 1 + 1 + 1 > 0.
#include <cstdio>
#include <cstring>
#include <vector>
#include "srs_check.hpp"

using ezkl::srs::FqPortable;

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s <cases>\n", argv[0]);
        return 2;
    }
    const FqPortable::fe one = FqPortable::one();
    if (!FqPortable::eq(FqPortable::mul(one, one), one)) {
        std::printf("FAIL: one * one != one\n");
        return 1;
    }
    const FqPortable::fe three = FqPortable::add(FqPortable::add(one, one), one);
    if (FqPortable::eq(three, one) || ezkl::srs::words_ge_q(three.v)) {
        std::printf("FAIL: 3 is not a reduced value other than 1\n");
        return 1;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    std::vector<unsigned char> buf;
    unsigned char chunk[4096];
    for (size_t got; (got = std::fread(chunk, 1, sizeof chunk, f)) > 0;) buf.insert(buf.end(), chunk, chunk + got);
    std::fclose(f);
    if (buf.empty() || buf.size() % 65) {
        std::printf("FAIL: %zu bytes is not a whole number of cases\n", buf.size());
        return 1;
    }
    const size_t n = buf.size() / 65;
    size_t by_reason[4] = {0, 0, 0, 0}, identities = 0;
    for (size_t i = 0; i < n; i++) {
        uint32_t w[16];
        std::memcpy(w, &buf[65 * i], 64);                 // the records sit at odd offsets: copied out, never read in place
        bool identity = false;
        const uint32_t reason = ezkl::srs::point_reason<FqPortable>(w, &identity);
        const unsigned want = buf[65 * i + 64];
        if (reason > 3 || (reason | (identity ? 4u : 0u)) != want) {
            std::printf("FAIL: case %zu: reason %u identity %d, the reference says reason %u identity %u\n", i, reason, (int)identity, want & 3, want >> 2);
            return 1;
        }
        by_reason[reason]++;
        identities += identity;
    }
    std::printf("%zu cases: %zu valid (%zu identities), %zu x >= q, %zu y >= q, %zu off the curve\n", n, by_reason[0], identities, by_reason[1], by_reason[2],
                by_reason[3]);
    std::printf("all checks passed\n");
    return 0;
}
