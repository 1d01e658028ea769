// srs_check.hpp -- is a 64-byte record of an SRS file a point of BN254 G1?  ONE predicate for the device kernel that walks a resident base set
// (g1_check_kernel, msm.hip), for the host prover's pairing entry point (ezkl_prover_srs_pairing_check) and for a plain CPU program
// (tests/cpp/test_srs_check.cpp).  Plain C++17 without HIP headers, in the manner of msm_plan.hpp.
//
// A record is the file's layout: x then y, each 8 x u32 little-endian limbs of a Montgomery Fq value (R = 2^256).  The verdict is what
// halo2's SerdeFormat::RawBytes reader decides: a range test on both coordinates (from_raw_bytes), then is_on_curve | is_identity.
//   0  valid            (all 64 bytes zero is the identity: valid, and flagged separately)
//   1  x >= q           as a 256-bit integer
//   2  y >= q
//   3  y^2 != x^3 + 3
// The first applicable code wins.  The equation is compared in Montgomery form -- both sides carry the same factor R, so nothing is
// converted; 3 is 3R mod q there.  BN254 G1 has cofactor 1 (the curve's order IS the prime r), so a point on the curve is in the group: there
// is no subgroup test to make.  (G2, on the twist, is another matter: see ezkl_prover_srs_pairing_check.)
//
// The arithmetic is a parameter: point_reason<F> works in any field class with the interface of field.hpp's Field<P> (one / add / mul / eq
// over a struct of 8 u32 limbs).  Device code passes ezkl::Fq, the radix-2^32 Fq of field.hpp; a program that cannot include field.hpp (it
// needs the HIP runtime's headers) passes FqPortable below, the same operand-scanning Montgomery product in plain C++.
#pragma once
#include <cstddef>
#include <cstdint>
#include "bn254_constants.h"
#if defined(__HIPCC__) || defined(__HIP__)
#define SRS_HD __host__ __device__
#else
#define SRS_HD
#endif

namespace ezkl {
namespace srs {

enum : uint32_t { POINT_OK = 0, POINT_X_RANGE = 1, POINT_Y_RANGE = 2, POINT_OFF_CURVE = 3 };

struct FqWords {
    static constexpr uint32_t MOD[8] = BN32_FQ_MOD_INIT;
    static constexpr uint32_t ONE[8] = BN32_FQ_R_INIT;
    static constexpr uint32_t INV = BN32_FQ_INV;
};

// a >= q as 256-bit integers: the subtraction a - q leaves no borrow
SRS_HD inline bool words_ge_q(const uint32_t* a) {
    uint32_t borrow = 0;
    for (int i = 0; i < 8; i++) {
        const uint64_t d = (uint64_t)a[i] - FqWords::MOD[i] - borrow;
        borrow = (uint32_t)(d >> 63);
    }
    return borrow == 0;
}

// Fq for a program without field.hpp: fully reduced Montgomery values, the interface point_reason needs and no more
struct FqPortable {
    struct fe {
        uint32_t v[8];
    };
    SRS_HD static fe one() {
        fe r;
        for (int i = 0; i < 8; i++) r.v[i] = FqWords::ONE[i];
        return r;
    }
    SRS_HD static bool eq(const fe& a, const fe& b) {
        uint32_t o = 0;
        for (int i = 0; i < 8; i++) o |= a.v[i] ^ b.v[i];
        return o == 0;
    }
    SRS_HD static fe reduce_once(const fe& a) {             // a < 2q
        if (!words_ge_q(a.v)) return a;
        fe r;
        uint32_t borrow = 0;
        for (int i = 0; i < 8; i++) {
            const uint64_t d = (uint64_t)a.v[i] - FqWords::MOD[i] - borrow;
            r.v[i] = (uint32_t)d;
            borrow = (uint32_t)(d >> 63);
        }
        return r;
    }
    SRS_HD static fe add(const fe& a, const fe& b) {        // a + b < 2q < 2^255: no carry out of limb 7
        fe s;
        uint64_t c = 0;
        for (int i = 0; i < 8; i++) {
            c += (uint64_t)a.v[i] + b.v[i];
            s.v[i] = (uint32_t)c;
            c >>= 32;
        }
        return reduce_once(s);
    }
    // a b / R mod q, one row of b at a time with the reduction folded in: t = (t + a b[i] + m q) / 2^32 stays below 2q in 8 limbs
    // because the top limb of q is below 2^30
    SRS_HD static fe mul(const fe& a, const fe& b) {
        uint32_t t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = 0; i < 8; i++) {
            const uint32_t bi = b.v[i];
            uint64_t A = (uint64_t)a.v[0] * bi + t[0];
            const uint32_t m = (uint32_t)A * FqWords::INV;
            uint64_t C = (uint64_t)m * FqWords::MOD[0] + (uint32_t)A;
            for (int j = 1; j < 8; j++) {
                A = (uint64_t)a.v[j] * bi + t[j] + (A >> 32);
                C = (uint64_t)m * FqWords::MOD[j] + (uint32_t)A + (C >> 32);
                t[j - 1] = (uint32_t)C;
            }
            t[7] = (uint32_t)(A >> 32) + (uint32_t)(C >> 32);
        }
        fe r;
        for (int i = 0; i < 8; i++) r.v[i] = t[i];
        return reduce_once(r);
    }
};

// the verdict on one record of 16 words; *identity says whether it is the all-zero record
template <class F>
SRS_HD inline uint32_t point_reason(const uint32_t* w, bool* identity) {
    uint32_t any = 0;
    for (int i = 0; i < 16; i++) any |= w[i];
    *identity = any == 0;
    if (!any) return POINT_OK;
    if (words_ge_q(w)) return POINT_X_RANGE;
    if (words_ge_q(w + 8)) return POINT_Y_RANGE;
    auto x = F::one(), y = x;
    for (int i = 0; i < 8; i++) {
        x.v[i] = w[i];
        y.v[i] = w[8 + i];
    }
    const auto one = F::one();
    const auto three = F::add(F::add(one, one), one);
    const auto rhs = F::add(F::mul(F::mul(x, x), x), three);
    return F::eq(F::mul(y, y), rhs) ? POINT_OK : POINT_OFF_CURVE;
}

}  // namespace srs
}  // namespace ezkl
