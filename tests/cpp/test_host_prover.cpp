// The host-only part of the prover -- the code that reads bytes from outside: circuit blobs, key files, proofs, witness plans -- as a
// plain program, so that it runs under AddressSanitizer / UndefinedBehaviorSanitizer without a device and without a library loaded into
// an interpreter (tests/test_host_prover_cpp.py builds and runs it).  It links nothing but the C++ runtime: the one C-ABI symbol the
// headers need is the stub below.
//
//   test_host_prover DIR [STRIDE [EVAL_STEP]]
//   test_host_prover DIR evaluations
// DIR: the inputs the Python test writes.  STRIDE thins the single-byte sweeps (every STRIDE-th byte; choose it coprime to the 4-byte
// words and 48-byte node records of the blob, so that every byte position of both is visited), EVAL_STEP the bit flips in the proof's
// evaluations (every EVAL_STEP-th bit); both default to 1, the complete sweeps.  Truncations and the bit flips in the proof's points
// are always complete.  `evaluations`: nothing but EVERY bit flip in the proof's evaluations -- each a whole verification, which is
// why the Python test runs this mode from a build without the sanitizers.
//
// An outcome is asserted only where it is certain; everywhere else the check is "returns or throws Error", and the sanitizers'.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <atomic>
#include <set>
#include <thread>
#include "cs.hpp"
#include "keyfile.hpp"
#include "verify.hpp"
#include "../witness_plan.hpp"

extern "C" const char* ezkl_hip_strerror(int) { return "refused"; }

using namespace ezkl_prover;
using Bytes = std::vector<uint8_t>;

static std::atomic<int> g_failures{0};
static void expect(bool ok, const char* what, long at = -1) {
    if (ok) return;
    if (++g_failures <= 20) fprintf(stderr, "FAILED: %s (at %ld)\n", what, at);
}
// cases [0, n) over a few threads: they are independent of each other, and the sanitizers make each several times slower
template <class F>
static void sweep(size_t n, F&& one) {
    const size_t T = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    std::vector<std::thread> th;
    for (size_t t = 0; t < T; t++)
        th.emplace_back([&, t] {
            for (size_t i = t; i < n; i += T) one(i);
        });
    for (auto& x : th) x.join();
}
static Bytes flipped(Bytes b, size_t bit) {
    b[bit / 8] ^= (uint8_t)(1u << (bit % 8));
    return b;
}
static Bytes slurp(const std::string& dir, const char* name) {
    std::ifstream f(dir + "/" + name, std::ios::binary);
    if (!f) { fprintf(stderr, "cannot read %s/%s\n", dir.c_str(), name); exit(2); }
    return Bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
// a copy of exactly `len` bytes on the heap: a read past the end is the sanitizer's to find
static Bytes head(const Bytes& b, size_t len) { return Bytes(b.begin(), b.begin() + len); }
static double seconds() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Instances {
    std::vector<Bytes> cols;                   // 32-byte Montgomery values
    std::vector<const void*> ptrs;
    std::vector<uint32_t> lens;
    void point() {
        ptrs.clear(); lens.clear();
        for (auto& c : cols) { ptrs.push_back(c.data()); lens.push_back((uint32_t)(c.size() / 32)); }
        if (ptrs.empty()) { ptrs.push_back(nullptr); lens.push_back(0); }
    }
};
enum Outcome { ACCEPTED, REJECTED, REFUSED };
static thread_local std::string g_why;
static Outcome verify(const VerifyingKey& vk, const Bytes& g2, const Bytes& s_g2, const Bytes& proof, const Instances& inst) {
    try {
        return verify_with(vk, g2.data(), s_g2.data(), proof.data(), proof.size(), inst.ptrs.data(), inst.lens.data(), g_why) ? ACCEPTED : REJECTED;
    } catch (const Error& e) {
        g_why = e.what();
        return REFUSED;
    }
}
static Outcome verify_from_key(ConstraintSystem& cs, const Bytes& key, const Bytes& g2, const Bytes& s_g2, const Bytes& proof, const Instances& inst) {
    try {
        return verify(vk_read(cs, key.data(), key.size()), g2, s_g2, proof, inst);
    } catch (const Error& e) {
        g_why = e.what();
        return REFUSED;
    }
}
template <class F>
static bool refused(F&& f) {
    try {
        f();
        return false;
    } catch (const Error& e) {
        g_why = e.what();
        return true;
    }
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: test_host_prover DIR [STRIDE [EVAL_STEP]] | DIR evaluations\n"); return 2; }
    const std::string dir = argv[1];
    const bool only_evaluations = argc > 2 && std::string(argv[2]) == "evaluations";
    const size_t stride = argc > 2 && !only_evaluations ? (size_t)atol(argv[2]) : 1, eval_step = argc > 3 ? (size_t)atol(argv[3]) : 1;
    double t0 = seconds();
    auto lap = [&](const char* what, size_t cases) {
        const double t = seconds();
        printf("%-28s %8zu cases %7.2f s\n", what, cases, t - t0);
        fflush(stdout);
        t0 = t;
    };
    const Bytes blob = slurp(dir, "cs.blob"), vk = slurp(dir, "vk.key"), proof = slurp(dir, "proof.bin"), g2 = slurp(dir, "g2.bin"), s_g2 = slurp(dir, "s_g2.bin");
    auto cs = parse_cs(blob.data(), blob.size());
    Instances inst;
    {
        const Bytes raw = slurp(dir, "instances.bin");              // u32 columns | per column: u32 rows | rows x 32 bytes
        Reader r{raw.data(), raw.size()};
        for (uint32_t c = r.u32(); c-- > 0;) {
            inst.cols.emplace_back(32 * (size_t)r.u32());
            r.bytes(inst.cols.back().data(), inst.cols.back().size());
        }
        inst.point();
    }
    std::atomic<size_t> cases{0};

    // ---- the proof
    const VerifyingKey key = vk_read(*cs, vk.data(), vk.size());
    expect(verify(key, g2, s_g2, proof, inst) == ACCEPTED, "the valid proof is accepted");
    if (!only_evaluations) {
    expect(verify(key, s_g2, g2, proof, inst) == REJECTED, "g2 and s_g2 swapped: rejected");
    {
        Instances other = inst;
        const Fe one = Fe::one();
        std::memcpy(other.cols.at(0).data(), one.v.data(), 32);
        other.point();
        expect(std::memcmp(other.cols[0].data(), inst.cols[0].data(), 32) != 0, "the fixture's first public value is not 1");
        expect(verify(key, g2, s_g2, proof, other) == REJECTED, "other instance values: rejected");
        other.cols[0].resize(other.cols[0].size() - 32);
        other.point();
        expect(verify(key, g2, s_g2, proof, other) == REJECTED, "one instance value fewer: rejected");
    }
    lap("proof: valid, g2, instances", 4);
    sweep(proof.size(), [&](size_t len) { expect(verify(key, g2, s_g2, head(proof, len), inst) == REJECTED, "a truncated proof is rejected", (long)len); });
    {
        Bytes longer = proof;
        longer.insert(longer.end(), 32, 0);
        expect(verify(key, g2, s_g2, longer, inst) == REJECTED, "a proof with 32 bytes behind it is rejected");
    }
    lap("proof: truncations", proof.size() + 1);
    }
    {
        // Commitments first, then the evaluations, then the two points of the opening.  A flipped bit in a point is rejected where the
        // point is read (it is no longer on the curve); one in an evaluation only by the pairing at the very end, a whole verification
        const size_t nl = cs->lookups.size(), points = cs->n_advice + nl + cs->n_chunks + nl + 1 + (cs->degree - 1);
        const size_t scalars = cs->advice_queries.size() + cs->fixed_queries.size() + 1 + cs->perm.size() + (cs->n_chunks ? 3 * cs->n_chunks - 1 : 0) + 3 * nl;
        const size_t ev_lo = 8 * 64 * points, ev_hi = ev_lo + 8 * 32 * scalars;
        expect(ev_hi + 8 * 128 == 8 * proof.size(), "the proof is its commitments, its evaluations and two opening points");
        sweep(8 * proof.size(), [&](size_t bit) {
            if (only_evaluations ? bit < ev_lo || bit >= ev_hi : bit >= ev_lo && bit < ev_hi && (bit - ev_lo) % eval_step) return;
            expect(verify(key, g2, s_g2, flipped(proof, bit), inst) == REJECTED, "a proof with one bit flipped is rejected", (long)bit);
            cases++;
        });
        lap(only_evaluations ? "proof: every evaluation bit" : "proof: single-bit flips", cases);
    }
    if (only_evaluations) {
        if (g_failures) return 1;
        printf("all checks passed\n");
        return 0;
    }

    // ---- the verifying key
    const size_t commitments = 64 * ((size_t)cs->n_fixed + cs->perm.size()), vk_len = 7 + commitments + (size_t)cs->n_selectors * ((cs->n + 7) / 8);
    expect(vk.size() == vk_len, "the vk.key is header + commitments + selector section");
    sweep(vk_len, [&](size_t len) {
        const Outcome o = verify_from_key(*cs, head(vk, len), g2, s_g2, proof, inst);
        expect(o == REFUSED && g_why.find("truncated") != std::string::npos, "a truncated verifying key is refused as truncated", (long)len);
    });
    lap("vk: truncations", vk_len);
    cases = 0;
    sweep(8 * (7 + commitments), [&](size_t bit) {
        if (bit / 8 == 2) return;
        expect(verify_from_key(*cs, flipped(vk, bit), g2, s_g2, proof, inst) != ACCEPTED, "a flipped bit in the header or the commitments: refused or rejected", (long)bit);
        cases++;
    });
    lap("vk: header, commitments", cases);
    {
        // byte 2 and the selector section are not bound into the digest: a flip there must not change the answer
        std::vector<size_t> bits = {16, 17, 18, 19, 20, 21, 22, 23};
        for (size_t bit = 8 * (7 + commitments); bit < 8 * vk_len; bit += stride) bits.push_back(bit);      // every STRIDE-th BIT: each is a whole verification
        sweep(bits.size(), [&](size_t i) {
            expect(verify_from_key(*cs, flipped(vk, bits[i]), g2, s_g2, proof, inst) == ACCEPTED, "a flipped bit in byte 2 or the selector section: still accepted", (long)bits[i]);
        });
        lap("vk: byte 2, selectors", bits.size());
        // wrong in two ways: the walker checks the headers and lengths before anybody looks at a commitment, so the length is what is named
        Bytes both = flipped(head(vk, vk_len - 1), 8 * 7 + 3);
        expect(verify_from_key(*cs, both, g2, s_g2, proof, inst) == REFUSED && g_why.find("verifying key truncated (selector section)") != std::string::npos,
               "a bad commitment in a key whose selector section is cut: refused as truncated");
        both = head(flipped(vk, 8), 7 + commitments - 1);
        expect(verify_from_key(*cs, both, g2, s_g2, proof, inst) == REFUSED && g_why.find("verifying key truncated") != std::string::npos,
               "another k in a key cut inside its commitments: refused as truncated");
    }

    // ---- the proving key: the reference's own k = 6 files, under the same constraint system
    {
        const Bytes pk = slurp(dir, "pk_k6.key"), gvk = slurp(dir, "vk_k6.key"), fixed = slurp(dir, "fixed_values.bin"), fixed_idx = slurp(dir, "fixed_idx.bin");
        const KeyLayout at = walk_key(*cs, pk.data(), pk.size(), true);
        const size_t n = cs->n, ne = (size_t)1 << cs->ext_k;
        std::set<size_t> bounds = {0, 7};
        size_t next = 7;
        expect(at.fixed_commitments == next, "fixed commitments follow the header");
        next += 64 * (size_t)cs->n_fixed; bounds.insert(next);
        expect(at.sigma_commitments == next, "permutation commitments follow");
        next += 64 * cs->perm.size(); bounds.insert(next);
        expect(at.selectors == next && at.selector_bytes == vk_len - next, "the selector section follows");
        next += at.selector_bytes; bounds.insert(next);
        auto poly = [&](const KeySection& s, size_t rows) {
            expect(s.off == next + 4 && s.rows == rows, "a polynomial: its length word, then its rows", (long)next);
            bounds.insert(next + 4);
            next += 4 + 32 * rows; bounds.insert(next);
        };
        auto vec = [&](const std::vector<KeySection>& v, size_t count, size_t rows) {
            expect(v.size() == count, "a vector has one section per column", (long)next);
            next += 4 + 4 * count; bounds.insert(next);
            for (auto& s : v) poly(s, rows);
        };
        poly(at.l0, ne); poly(at.l_last, ne); poly(at.l_active_row, ne);
        vec(at.fixed_values, cs->n_fixed, n); vec(at.fixed_polys, cs->n_fixed, n); vec(at.fixed_cosets, cs->n_fixed, ne);
        vec(at.permutations, cs->perm.size(), n); vec(at.perm_polys, cs->perm.size(), n); vec(at.perm_cosets, cs->perm.size(), ne);
        expect(next == pk.size() && at.end == pk.size(), "the sections tile the file exactly");
        for (size_t i = 0; i < fixed_idx.size() / 4; i++) {
            uint32_t c;
            std::memcpy(&c, fixed_idx.data() + 4 * i, 4);
            expect(c < at.fixed_values.size() && std::memcmp(pk.data() + at.fixed_values[c].off, fixed.data() + 32 * n * i, 32 * n) == 0,
                   "fixed_values[c] are the bytes of the exported fixture column", (long)c);
        }
        std::set<size_t> cuts;
        for (size_t b : bounds)
            for (size_t len : {b - 1, b, b + 1})
                if (len < pk.size()) cuts.insert(len);               // b = 0: b - 1 wraps round
        const std::vector<size_t> lens(cuts.begin(), cuts.end());
        sweep(lens.size(), [&](size_t i) {
            const Bytes cut = head(pk, lens[i]);
            expect(refused([&] { walk_key(*cs, cut.data(), cut.size(), true); }), "a proving key cut at or beside a section boundary is refused", (long)lens[i]);
        });
        {
            // wrong in two ways: a polynomial of another length in the LAST section and a non-canonical element in the first.  The walker
            // reads no element, so whoever consumes the bytes hears of the header first
            Bytes both = pk;
            std::memset(both.data() + at.l0.off, 0xff, 32);
            both[at.perm_cosets.back().off - 1] ^= 1;
            expect(refused([&] { walk_key(*cs, both.data(), both.size(), true); }) && g_why.find("polynomial of unexpected length in the key") != std::string::npos,
                   "the walker names a header fault whatever the elements before it hold");
        }
        Bytes longer = pk;
        longer.push_back(0);
        expect(refused([&] { walk_key(*cs, longer.data(), longer.size(), true); }) && g_why.find("trailing bytes") != std::string::npos, "one trailing byte is refused");
        const KeyLayout v = walk_key(*cs, gvk.data(), gvk.size(), false), p = walk_key(*cs, pk.data(), pk.size(), false);
        expect(v.end == gvk.size() && p.end == gvk.size() && v.selectors == p.selectors && std::memcmp(pk.data(), gvk.data(), gvk.size()) == 0,
               "vk_k6.key walks as a verifying key, and as the prefix of pk_k6.key");
        (void)vk_read(*cs, gvk.data(), gvk.size());                 // its commitments are points of the curve
        lap("pk: layout, boundaries", lens.size() + 3);
    }

    // ---- the circuit blob
    sweep(blob.size(), [&](size_t len) {
        const Bytes cut = head(blob, len);
        expect(refused([&] { parse_cs(cut.data(), cut.size()); }), "a truncated circuit blob is refused", (long)len);
    });
    lap("blob: truncations", blob.size());
    sweep((blob.size() + stride - 1) / stride, [&](size_t j) {                 // parses or is refused
        for (uint8_t x : {(uint8_t)(1u << (j % 8)), (uint8_t)0xff}) {
            Bytes bad = blob;
            bad[j * stride] ^= x;
            (void)refused([&] { parse_cs(bad.data(), bad.size()); });
        }
    });
    lap("blob: single-byte changes", 2 * ((blob.size() + stride - 1) / stride));

    // ---- the witness plan
    {
        const Bytes plan = slurp(dir, "plan.blob");
        ezkl::wplan::Plan out;
        std::string why;
        expect(ezkl::wplan::parse(plan.data(), plan.size(), out, why), "the valid witness plan parses");
        sweep(plan.size(), [&](size_t len) {
            const Bytes cut = head(plan, len);
            ezkl::wplan::Plan o;
            std::string w;
            expect(!ezkl::wplan::parse(cut.data(), cut.size(), o, w), "a truncated witness plan is refused", (long)len);
        });
        lap("plan: truncations", plan.size());
        uint32_t h[20];
        std::memcpy(h, plan.data(), sizeof h);
        const size_t records = sizeof h + 32 + 8 * (size_t)h[6] + 32 * (size_t)h[7], stop = std::min(plan.size(), records + 32 * std::min<size_t>(h[4], 64));
        std::vector<size_t> at;                                     // the header, then the first 64 records
        for (size_t i = 0; i < sizeof h + 32; i++) at.push_back(i);
        for (size_t i = records; i < stop; i++) at.push_back(i);
        sweep(at.size(), [&](size_t j) {                            // parses or is refused
            for (uint8_t x : {(uint8_t)(1u << (j % 8)), (uint8_t)0xff}) {
                Bytes bad = plan;
                bad[at[j]] ^= x;
                ezkl::wplan::Plan o;
                std::string w;
                (void)ezkl::wplan::parse(bad.data(), bad.size(), o, w);
            }
        });
        lap("plan: single-byte changes", 2 * at.size());
    }
    if (g_failures) {
        fprintf(stderr, "%d checks failed\n", g_failures.load());
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
