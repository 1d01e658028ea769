// One walker for the key files (halo2 ProvingKey::{write, read}, SerdeFormat::RawBytes), the layout of the reference's vk.key / pk.key
// (verified on its test assets in SURVEY.md §8(c) item 3):
//   VK = [3, k, compress_selectors] | u32 LE #fixed | #fixed x G1 | #perm x G1 | selectors (n_selectors x n / 8 bytes: bit-packed rows;
//        halo2 does not store their count: it re-runs configure, here the constraint system carries it)
//   PK = VK | poly l0 | poly l_last | poly l_active_row | vec fixed_values | vec fixed_polys | vec fixed_cosets | vec permutations |
//        vec perm_polys | vec perm_cosets
// with poly = u32 BE len | len x 32 B and vec = u32 BE count | count x u32 BE len | count x poly.  Field and curve bytes are the resident
// Montgomery bytes, copied unchanged in both directions.
// The walker reads HEADERS only -- a k = 20 key is a 7.8 GB mapping whose section bodies must not be faulted in -- and says where things
// are; whether a section's elements are canonical residues (or points of the curve) is checked by whoever consumes its bytes.
#pragma once
#include "cs.hpp"

namespace ezkl_prover {

struct KeySection {
    size_t off = 0, rows = 0;       // `rows` elements of 32 bytes from byte `off` on (behind the polynomial's own length word)
};
struct KeyLayout {
    size_t fixed_commitments = 0, sigma_commitments = 0;      // cs.n_fixed and cs.perm.size() points of 64 bytes
    size_t selectors = 0, selector_bytes = 0;
    KeySection l0, l_last, l_active_row;                      // a proving key only, like the vectors
    std::vector<KeySection> fixed_values, fixed_polys, fixed_cosets, permutations, perm_polys, perm_cosets;
    size_t end = 0;                                           // the first byte behind what was walked
};
// proving_key = false: the verifying key, which ends behind the selector section; a pk.key -- whose prefix the vk is -- is accepted
inline KeyLayout walk_key(const ConstraintSystem& cs, const uint8_t* buf, size_t len, bool proving_key) {
    KeyLayout at;
    const size_t nf = cs.n_fixed, np = cs.perm.size(), n = cs.n, ne = (size_t)1 << cs.ext_k;
    const char* truncated = proving_key ? "proving key truncated" : "verifying key truncated";
    size_t off = 0;
    auto need = [&](size_t m, const char* what) { invalid(off + m > len, what); };
    need(proving_key ? 7 : 7 + 64 * (nf + np), truncated);
    invalid(buf[0] != 3, "unsupported key version");
    invalid(buf[1] != cs.k, "key was made for another k");
    uint32_t file_nf = 0;
    for (int i = 0; i < 4; i++) file_nf |= (uint32_t)buf[3 + i] << (8 * i);
    invalid(file_nf != nf, "key has another number of fixed columns");
    off = 7;
    need(64 * (nf + np), truncated);
    at.fixed_commitments = off;
    at.sigma_commitments = off + 64 * nf;
    off += 64 * (nf + np);
    at.selectors = off;
    at.selector_bytes = (size_t)cs.n_selectors * ((cs.n + 7) / 8);
    need(at.selector_bytes, proving_key ? truncated : "verifying key truncated (selector section)");
    at.end = off += at.selector_bytes;
    if (!proving_key) return at;
    auto be32 = [&]() {
        need(4, truncated);
        uint32_t v = ((uint32_t)buf[off] << 24) | ((uint32_t)buf[off + 1] << 16) | ((uint32_t)buf[off + 2] << 8) | buf[off + 3];
        off += 4;
        return v;
    };
    auto poly = [&](size_t m) {
        invalid(be32() != m, "polynomial of unexpected length in the key");
        need(32 * m, truncated);
        const KeySection s{off, m};
        off += 32 * m;
        return s;
    };
    auto vec = [&](std::vector<KeySection>& out, size_t count, size_t m) {
        invalid(be32() != count, "vector of unexpected length in the key");
        for (size_t i = 0; i < count; i++) invalid(be32() != m, "polynomial of unexpected length in the key");
        for (size_t i = 0; i < count; i++) out.push_back(poly(m));
    };
    at.l0 = poly(ne); at.l_last = poly(ne); at.l_active_row = poly(ne);
    vec(at.fixed_values, nf, n); vec(at.fixed_polys, nf, n); vec(at.fixed_cosets, nf, ne);
    vec(at.permutations, np, n); vec(at.perm_polys, np, n); vec(at.perm_cosets, np, ne);
    invalid(off != len, "trailing bytes in the proving key");
    at.end = off;
    return at;
}

}  // namespace ezkl_prover
