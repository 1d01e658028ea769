// The compressed-point encoding table of ezkl_amd/csrc/g1_encoding.hpp as a plain program (no device, no HIP headers), built by
// tests/test_g1_compress_cpu.py under AddressSanitizer and UndefinedBehaviorSanitizer.
//
//   test_g1_encoding <cases>   cases: records of 34 bytes -- a 32-byte encoding, then what tests/g1_compress_ref.py says of it before any
//                              field arithmetic: the verdict of split() (0, 1 or 4), then sign | identity << 1
// Every record goes through split(); a valid one is put together again with join() / identity() and must come back byte for byte.
#include <cstdio>
#include <cstring>
#include <vector>
#include "g1_encoding.hpp"

int main(int argc, char** argv) {
    std::FILE* f = argc == 2 ? std::fopen(argv[1], "rb") : nullptr;
    if (!f) {
        std::fprintf(stderr, "usage: %s <cases>\n", argv[0]);
        return 2;
    }
    std::vector<unsigned char> buf;
    unsigned char chunk[4096];
    for (size_t got; (got = std::fread(chunk, 1, sizeof chunk, f)) > 0;) buf.insert(buf.end(), chunk, chunk + got);
    std::fclose(f);
    if (buf.empty() || buf.size() % 34) {
        std::printf("FAIL: %zu bytes is not a whole number of cases\n", buf.size());
        return 1;
    }
    const size_t n = buf.size() / 34;
    for (size_t i = 0; i < n; i++) {
        uint32_t w[8], back[8];
        std::memcpy(w, &buf[34 * i], 32);                 // copied out: the records sit at unaligned offsets
        bool sign = false, identity = false;
        const uint32_t verdict = ezkl::g1enc::split(w, &sign, &identity);
        const unsigned want = buf[34 * i + 32], flags = buf[34 * i + 33];
        if (verdict != want || (unsigned)sign != (flags & 1) || (unsigned)identity != flags >> 1) {
            std::printf("FAIL: case %zu: verdict %u sign %d identity %d, the reference says %u %u %u\n", i, verdict, (int)sign, (int)identity, want, flags & 1,
                        flags >> 1);
            return 1;
        }
        if (verdict) continue;
        std::memcpy(back, w, 32);
        if (identity) ezkl::g1enc::identity(back);
        else ezkl::g1enc::join(back, sign);
        if (std::memcmp(back, &buf[34 * i], 32)) {
            std::printf("FAIL: case %zu does not come back from split() and join()\n", i);
            return 1;
        }
    }
    std::printf("%zu cases: all checks passed\n", n);
    return 0;
}
