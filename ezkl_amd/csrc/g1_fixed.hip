// g1_fixed.hip -- out[i] = scalars[i] * P for ONE point P: a windowed comb over a table of P's multiples (SRS generation: g[i] = s^i G,
// g_lagrange[i] = L_i(s) G both multiply the generator).
//
// The double-and-add kernel (msm.hip: g1_mul_fixed_kernel) spends ~254 doublings, ~127 additions and an inversion of its own on every scalar
// and never uses that the point is the same in every lane.  Here the doublings are done once per call:
//   rows    B_w = 2^(c w) P for the W = ceil(254 / c) windows: a serial chain of c (W - 1) doublings, one wave
//   table   T[w][d - 1] = d B_w for d = 1 .. 2^(c-1), one lane per entry, affine 64-byte records (shared inversion, below)
//   comb    one lane per scalar: signed digits d_w in [-2^(c-1), 2^(c-1)], s = sum_w d_w 2^(c w); the lane adds sign(d_w) T[w][|d_w| - 1]
//           for every non-zero digit -- W mixed additions at the most, no doubling -- and normalises with a shared inversion
// The table (W 2^(c-1) records: 832 KiB at c = 10) is gathered from L2, 64 bytes per digit; it does not fit in LDS.
//
// Shared inversion (g1x_to_affine_shared): a lane needs 1 / ZZZ.  The lanes that share one inversion multiply their ZZZ together by a
// butterfly of lane shuffles -- after level k every lane holds the product of its aligned group of 2^(k+1) lanes and keeps the sibling
// group's product it was multiplied by -- the total is inverted ONCE, and the way down multiplies the inverse by the kept sibling products,
// level by level: 1 / (a b) * b = 1 / a.  12 products per lane and a share of one Fermat inversion (~380 products) in place of a whole one.
// The four waves of a workgroup pool their totals through LDS and the first wave inverts for all of them: MEASURED against an inversion per
// wave, 2^20 scalars at c = 8: 6.2 against 7.8 ms (tools/fixed_base_bench.py).
#include "common.hpp"
#include "curve.hpp"
#include "msm_plan.hpp"
#include <string.h>

namespace ezkl {

static constexpr uint32_t FB_C = G1_FIXED_C, FB_W = G1_FIXED_WINDOWS, FB_HALF = 1u << (FB_C - 1), FB_ENTRIES = FB_W * FB_HALF;
static constexpr uint32_t FB_THREADS = 256, FB_WAVES = FB_THREADS / 64;
// The top window holds 254 - c (W - 1) = 254 mod c bits.  A canonical scalar is below r < 2^254, so the top window's bits are at most
// 2^(254 mod c) - 1, and with the carry from below its digit is at most 2^(254 mod c) <= 2^(c-1) whenever 254 mod c is not 0: the digit
// is in the table and no carry leaves the top window.
static_assert(254 % FB_C != 0 && FB_C >= 2 && FB_C <= 16, "the top window must be shorter than c bits");

EZ_D fe_t fe_shfl_xor(const fe_t& a, uint32_t mask) {
    fe_t r;
#pragma unroll
    for (int k = 0; k < 8; k++) r.v[k] = __shfl_xor(a.v[k], mask);
    return r;
}

// Canonical affine form of p in every lane of a 256-thread workgroup, EVERY lane of which calls this (lanes without work pass the identity):
// the identity contributes 1 to the products and comes out as the all-zero record.  sh: FB_WAVES + 1 elements of LDS.
EZ_D g1a_t g1x_to_affine_shared(const g1x_t& p, fe_t* sh) {
    const bool id = g1x_is_id(p);
    fe_t t = id ? Fq::one() : p.zzz;
    fe_t sib[6];
#pragma unroll
    for (int k = 0; k < 6; k++) {
        sib[k] = fe_shfl_xor(t, 1u << k);
        t = Fq::mul(t, sib[k]);
    }
    // t: the product over the wave, in every lane
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) sh[wave] = t;
    __syncthreads();
    if (wave == 0) {                                      // ONE inversion per workgroup, by its first wave
        fe_t all = sh[0];
#pragma unroll
        for (uint32_t j = 1; j < FB_WAVES; j++) all = Fq::mul(all, sh[j]);
        all = Fq::inv(all);
        if (threadIdx.x == 0) sh[FB_WAVES] = all;
    }
    __syncthreads();
    fe_t inv = sh[FB_WAVES];                              // 1 / (every wave's total); times the OTHER waves' totals: 1 / this wave's
#pragma unroll 1
    for (uint32_t j = 0; j < FB_WAVES; j++)
        if (j != wave) inv = Fq::mul(inv, sh[j]);
#pragma unroll
    for (int k = 5; k >= 0; k--) inv = Fq::mul(inv, sib[k]);
    // inv = 1 / ZZZ.  ZZ = Z^2 and ZZZ = Z^3: 1 / Z = ZZ / ZZZ, x = X / Z^2, y = Y / ZZZ
    g1a_t r;
    const fe_t iz = Fq::mul(p.zz, inv);
    r.x = Fq::mul(p.x, Fq::sqr(iz));
    r.y = Fq::mul(p.y, inv);
    if (id) { r.x = Fq::zero(); r.y = Fq::zero(); }
    return r;
}

// rows[w] = 2^(c w) P in XYZZ.  The chain is serial; all 64 lanes of the one wave run it (a chain of field products is slower with most
// lanes masked off, curve.hpp: g1x_group_sum) and lane 0 stores.  An identity P gives identity rows.
__global__ __launch_bounds__(64) void g1_fixed_rows_kernel(g1a_t base, g1x_t* rows) {
    g1x_t b = g1x_from_affine(base);
#pragma unroll 1
    for (uint32_t w = 0; w < FB_W; w++) {
        if (threadIdx.x == 0) st_g1x(rows + w, b);
        if (w + 1 < FB_W) {
#pragma unroll 1
            for (uint32_t k = 0; k < FB_C; k++) b = g1x_double(b);
        }
    }
}

// table[w * 2^(c-1) + d - 1] = d rows[w], affine.  One lane per entry: double-and-add over the bits of d below its top one (at most c - 1
// doublings and additions; d rows[w] with d >= 2 never meets rows[w] itself while P has order r, and g1x_add is complete anyway).
__global__ __launch_bounds__(FB_THREADS) void g1_fixed_table_kernel(const g1x_t* rows, g1a_t* table) {
    __shared__ fe_t sh[FB_WAVES + 1];
    const uint32_t e = blockIdx.x * FB_THREADS + threadIdx.x;
    g1x_t acc = g1x_identity();
    if (e < FB_ENTRIES) {
        const uint32_t d = (e & (FB_HALF - 1)) + 1;
        const g1x_t b = ld_g1x(rows + (e >> (FB_C - 1)));
        acc = b;
#pragma unroll 1
        for (int bit = 30 - __clz(d); bit >= 0; bit--) {
            acc = g1x_double(acc);
            if ((d >> bit) & 1) acc = g1x_add(acc, b);
        }
    }
    const g1a_t a = g1x_to_affine_shared(acc, sh);
    if (e < FB_ENTRIES) st_g1a(table + e, a);
}

// out[i] = scalars[i] * P from P's table.  The scalar leaves Montgomery form and is recoded on the fly, LOWEST window first: the window's c
// bits plus the carry from below; a value above 2^(c-1) becomes value - 2^c with a carry upward (a value of exactly 2^(c-1) stays positive:
// it is the table's last entry).  Why lowest first: after windows 0 .. w-1 the partial sum is m P with |m| <= 2^(c-1) (2^(c w) - 1) / (2^c - 1)
// < 2^(c w), and the entry added next is +-d 2^(c w) P with d >= 1 -- as INTEGERS the two never agree up to sign, so the mixed addition
// sees neither equal nor opposite operands, and an identity accumulator only before the first non-zero digit.  Modulo r that holds in
// every window but the top one, where |m -+ d 2^(c w)| can reach r (s = 3 * 2^253 - r at c = 10 ends in the doubling 12 * 2^250 P +
// 12 * 2^250 P, since 24 * 2^250 = s + r); g1x_add_mixed tests for the doubling and the inverse and handles both, so the sum is right for
// every scalar and every P, of order r or not.
__global__ __launch_bounds__(FB_THREADS) void g1_fixed_comb_kernel(const g1a_t* __restrict__ table, const fe_t* __restrict__ scalars, size_t n,
                                                                   g1a_t* __restrict__ out) {
    __shared__ fe_t sh[FB_WAVES + 1];
    const size_t i = (size_t)blockIdx.x * FB_THREADS + threadIdx.x;
    g1x_t acc = g1x_identity();
    if (i < n) {
        fe_t s = Fr::redc(ld_fe(scalars + i));
        uint32_t carry = 0;
#pragma unroll 1
        for (uint32_t w = 0; w < FB_W; w++) {
            uint32_t v = (s.v[0] & ((1u << FB_C) - 1)) + carry;          // 0 .. 2^c
            carry = v > FB_HALF ? 1u : 0u;
            const bool neg = carry != 0;
            if (neg) v = (1u << FB_C) - v;                                // |digit|: 0 .. 2^(c-1)
#pragma unroll
            for (int j = 0; j < 7; j++) s.v[j] = (s.v[j] >> FB_C) | (s.v[j + 1] << (32 - FB_C));
            s.v[7] >>= FB_C;
            if (v) {
                g1a_t q = ld_g1a(table + (w * FB_HALF + v - 1));
                if (neg) q.y = Fq::neg(q.y);
                acc = g1x_add_mixed(acc, q);
            }
        }
    }
    // lanes past n stay in the barriers with the identity and store nothing
    const g1a_t a = g1x_to_affine_shared(acc, sh);
    if (i < n) st_g1a(out + i, a);
}

// The rows and the table live in the context's `aux` arena: grown on first use, kept between calls, handed from stream to stream by the
// arena's event.  HIP events: "fixed_base" around everything, "fixed_base_table" around the two table kernels.
int g1_fixed_base(Ctx* c, hipStream_t st, const void* base_host, const fe_t* scalars, size_t n, void* out_dev) {
    if (n == 0) return EZKL_OK;
    g1a_t b;
    memcpy(&b, base_host, 64);
    const size_t rows_bytes = FB_W * sizeof(g1x_t), table_bytes = (size_t)FB_ENTRIES * sizeof(g1a_t);
    uint8_t* S = nullptr;
    int rc = arena_reserve(c->aux, rows_bytes + table_bytes, st, (void**)&S);
    if (rc) return rc;
    g1x_t* rows = (g1x_t*)S;
    g1a_t* table = (g1a_t*)(S + rows_bytes);
    hipEvent_t e0, e1, t0, t1;
    if ((rc = ev_pair(c, "fixed_base", &e0, &e1))) return rc;
    if ((rc = ev_pair(c, "fixed_base_table", &t0, &t1))) return rc;
    EZ_HIP(hipEventRecord(e0, st));
    EZ_HIP(hipEventRecord(t0, st));
    hipLaunchKernelGGL(g1_fixed_rows_kernel, dim3(1), dim3(64), 0, st, b, rows);
    hipLaunchKernelGGL(g1_fixed_table_kernel, dim3(cdiv(FB_ENTRIES, FB_THREADS)), dim3(FB_THREADS), 0, st, (const g1x_t*)rows, table);
    EZ_HIP(hipGetLastError());
    EZ_HIP(hipEventRecord(t1, st));
    hipLaunchKernelGGL(g1_fixed_comb_kernel, dim3(cdiv(n, FB_THREADS)), dim3(FB_THREADS), 0, st, (const g1a_t*)table, scalars, n, (g1a_t*)out_dev);
    EZ_HIP(hipGetLastError());
    EZ_HIP(hipEventRecord(e1, st));
    return arena_done(c->aux, st);
}

}  // namespace ezkl
