// g1_encoding.hpp -- THE table of the compressed G1 encoding (halo2's SerdeFormat::Processed; halo2curves 0.7.0's GroupEncoding for bn256,
// a base field with two spare bits in its 32 bytes).  Both kernels of g1_compress.hip read it; ezkl_amd/codecs.py restates it
// (G1_SIGN_BIT, G1_IDENTITY_BIT) and tests/cpp/test_g1_encoding.cpp holds this file to that restatement.  Plain C++17 without HIP headers,
// in the manner of srs_check.hpp.
//
// A compressed point is 32 bytes: x as a canonical (NOT Montgomery) little-endian integer below q, with two flags in the spare bits of
// byte 31:
//   bit 254 of the integer = bit 6 of byte 31 (0x40)   sign: the parity of the canonical y, y mod 2
//   bit 255 of the integer = bit 7 of byte 31 (0x80)   identity: set for the point at infinity, whose x and sign bit are then zero
// As eight u32 little-endian words the flags are bits 30 and 31 of word 7.  A correction of the layout touches this file, codecs.py and
// nothing else.
//
// The verdict on an encoding, in the numbering of srs_check.hpp where the reasons coincide (the first applicable code wins):
//   0  valid
//   1  x >= q                       (POINT_X_RANGE)
//   3  x^3 + 3 is not a square      no point has this x (POINT_OFF_CURVE: the same comparison y^2 == x^3 + 3 decides it)
//   4  malformed flags              the identity flag with a non-zero x or with the sign bit
#pragma once
#include <cstdint>
#include "srs_check.hpp"

namespace ezkl {
namespace g1enc {

constexpr int SIGN_BIT = 254, IDENTITY_BIT = 255;
constexpr uint32_t SIGN_W7 = 1u << (SIGN_BIT - 224), IDENTITY_W7 = 1u << (IDENTITY_BIT - 224);
enum : uint32_t { ENC_OK = srs::POINT_OK, ENC_X_RANGE = srs::POINT_X_RANGE, ENC_NO_POINT = srs::POINT_OFF_CURVE, ENC_FLAGS = 4 };

// the eight words of an encoding -> x in w (flags cleared), the two flags, and the verdict as far as it can be had without arithmetic
// in the field: ENC_FLAGS, ENC_X_RANGE or ENC_OK ("decompress me", or the identity)
SRS_HD inline uint32_t split(uint32_t* w, bool* sign, bool* identity) {
    *sign = (w[7] & SIGN_W7) != 0;
    *identity = (w[7] & IDENTITY_W7) != 0;
    w[7] &= ~(SIGN_W7 | IDENTITY_W7);
    if (*identity) {
        uint32_t any = 0;
        for (int i = 0; i < 8; i++) any |= w[i];
        return any || *sign ? ENC_FLAGS : ENC_OK;
    }
    return srs::words_ge_q(w) ? ENC_X_RANGE : ENC_OK;
}
// canonical x, the parity of the canonical y -> the eight words
SRS_HD inline void join(uint32_t* w, bool y_odd) {
    if (y_odd) w[7] |= SIGN_W7;
}
SRS_HD inline void identity(uint32_t* w) {
    for (int i = 0; i < 7; i++) w[i] = 0;
    w[7] = IDENTITY_W7;
}

}  // namespace g1enc
}  // namespace ezkl
