// g2.hip -- BN254 G2 (the sextic twist y^2 = x^3 + 3 / (9 + u) over Fq2 = Fq[u] / (u^2 + 1)) on the device.
//
// On the prove path G2 is DATA (the two points g2 and s_g2 of the SRS file, consumed by the verifier's pairing); G2 sums are for SRS
// generation and update, and for callers that hold G2 points on the device (an SRS tail, G2 commitments of another protocol, the G2 powers of
// a powers-of-tau file).  Two paths:
//   * g2_msm_points_run: a signed-digit BUCKET chain over resident points and scalars.  The table-free G1 chain's sort front end
//     (msm_once_sort_enqueue, msm.hip) turns the scalars into per-window lists of (bucket, index) pairs; the kernels here are where the
//     group law lives: accumulate (one lane per bucket + a workgroup per long run), reduce (segments of buckets, then one workgroup per
//     window) and a tail that folds the windows and normalises on the device.  ~30 Fq products per (point, window) pair.  DESIGN.md §4.1
//     "G2 MSM"; the plan is msm_plan_g2 (msm_plan.hpp).
//   * g2_msm_partial_kernel / g2_msm_reduce_kernel: one double-and-add per (point, scalar) pair, ~4 000 Fq products each, a strided partial
//     sum per thread, one LDS tree.  ezkl_hip_msm_g2 (host pointers) keeps it below MSM_G2_CROSSOVER points -- n = 1 in gen_srs / update_srs.
// Field layer: field.hpp (radix 2^32, Fq::mul), not field29.hpp: the records arrive in the R = 2^256 Montgomery form of the SRS file and are
// consumed as they are (no conversion pass), an XYZZ accumulator over Fq2 is 64 VGPRs instead of 72, and every kernel here is bound by the
// latency of dependent products in few waves, not by the product throughput the radix-2^29 form was built for.
// Layout: a G2 affine point is the 128 bytes of the SRS file -- x.c0, x.c1, y.c0, y.c1, each a 32-byte little-endian Montgomery Fq --
// (0, 0) = identity.
#include "common.hpp"
#include "msm_plan.hpp"
#include <string.h>

namespace ezkl {

struct fq2_t {
    fe_t a, b;      // a + b u
};
struct g2a_t {
    fq2_t x, y;
};
struct g2j_t {      // Jacobian: x = X / Z^2, y = Y / Z^3; identity: Z = 0
    fq2_t x, y, z;
};

EZ_D fq2_t f2_zero() { return fq2_t{Fq::zero(), Fq::zero()}; }
EZ_D fq2_t f2_one() { return fq2_t{Fq::one(), Fq::zero()}; }
EZ_D bool f2_is_zero(const fq2_t& x) { return Fq::is_zero(x.a) && Fq::is_zero(x.b); }
EZ_D fq2_t f2_add(const fq2_t& x, const fq2_t& y) { return fq2_t{Fq::add(x.a, y.a), Fq::add(x.b, y.b)}; }
EZ_D fq2_t f2_sub(const fq2_t& x, const fq2_t& y) { return fq2_t{Fq::sub(x.a, y.a), Fq::sub(x.b, y.b)}; }
EZ_D fq2_t f2_dbl(const fq2_t& x) { return f2_add(x, x); }
EZ_D fq2_t f2_neg(const fq2_t& x) { return fq2_t{Fq::neg(x.a), Fq::neg(x.b)}; }
EZ_D fq2_t f2_mul(const fq2_t& x, const fq2_t& y) {                   // Karatsuba: 3 products
    const fe_t aa = Fq::mul(x.a, y.a), bb = Fq::mul(x.b, y.b);
    const fe_t cross = Fq::mul(Fq::add(x.a, x.b), Fq::add(y.a, y.b));
    return fq2_t{Fq::sub(aa, bb), Fq::sub(Fq::sub(cross, aa), bb)};
}
EZ_D fq2_t f2_sqr(const fq2_t& x) {                                    // (a + b)(a - b) + 2ab u: 2 products
    const fe_t t = Fq::mul(Fq::add(x.a, x.b), Fq::sub(x.a, x.b));
    const fe_t ab = Fq::mul(x.a, x.b);
    return fq2_t{t, Fq::dbl(ab)};
}
EZ_D fq2_t f2_inv(const fq2_t& x) {                                    // conj(x) / (a^2 + b^2)
    const fe_t n = Fq::inv(Fq::add(Fq::sqr(x.a), Fq::sqr(x.b)));
    return fq2_t{Fq::mul(x.a, n), Fq::neg(Fq::mul(x.b, n))};
}

EZ_D g2j_t g2_identity() { return g2j_t{f2_zero(), f2_zero(), f2_zero()}; }
EZ_D bool g2_is_id(const g2j_t& p) { return f2_is_zero(p.z); }
EZ_D g2j_t g2_from_affine(const g2a_t& p) {
    if (f2_is_zero(p.x) && f2_is_zero(p.y)) return g2_identity();
    return g2j_t{p.x, p.y, f2_one()};
}
// dbl-2009-l (a = 0)
EZ_D g2j_t g2_double(const g2j_t& p) {
    if (g2_is_id(p)) return p;
    const fq2_t A = f2_sqr(p.x), B = f2_sqr(p.y), C = f2_sqr(B);
    const fq2_t D = f2_dbl(f2_sub(f2_sub(f2_sqr(f2_add(p.x, B)), A), C));
    const fq2_t E = f2_add(f2_dbl(A), A), F = f2_sqr(E);
    g2j_t r;
    r.x = f2_sub(F, f2_dbl(D));
    const fq2_t C8 = f2_dbl(f2_dbl(f2_dbl(C)));
    r.y = f2_sub(f2_mul(E, f2_sub(D, r.x)), C8);
    r.z = f2_dbl(f2_mul(p.y, p.z));
    return r;
}
// add-2007-bl with the identity / doubling / inverse cases
EZ_D g2j_t g2_add(const g2j_t& p, const g2j_t& q) {
    if (g2_is_id(p)) return q;
    if (g2_is_id(q)) return p;
    const fq2_t z1z1 = f2_sqr(p.z), z2z2 = f2_sqr(q.z);
    const fq2_t u1 = f2_mul(p.x, z2z2), u2 = f2_mul(q.x, z1z1);
    const fq2_t s1 = f2_mul(f2_mul(p.y, q.z), z2z2), s2 = f2_mul(f2_mul(q.y, p.z), z1z1);
    const fq2_t h = f2_sub(u2, u1), rr = f2_dbl(f2_sub(s2, s1));
    if (f2_is_zero(h)) {
        if (f2_is_zero(rr)) return g2_double(p);
        return g2_identity();
    }
    const fq2_t i = f2_sqr(f2_dbl(h)), j = f2_mul(h, i), v = f2_mul(u1, i);
    g2j_t r;
    r.x = f2_sub(f2_sub(f2_sqr(rr), j), f2_dbl(v));
    r.y = f2_sub(f2_mul(rr, f2_sub(v, r.x)), f2_dbl(f2_mul(s1, j)));
    r.z = f2_mul(f2_sub(f2_sub(f2_sqr(f2_add(p.z, q.z)), z1z1), z2z2), h);
    return r;
}
EZ_D g2a_t g2_to_affine(const g2j_t& p) {
    if (g2_is_id(p)) return g2a_t{f2_zero(), f2_zero()};
    const fq2_t zi = f2_inv(p.z), zi2 = f2_sqr(zi);
    return g2a_t{f2_mul(p.x, zi2), f2_mul(p.y, f2_mul(zi2, zi))};
}
EZ_D g2j_t g2_scalar_mul(const g2j_t& p, const fe_t& s_canon) {
    g2j_t acc = g2_identity();
    bool started = false;
#pragma unroll 1
    for (int b = 253; b >= 0; b--) {
        if (started) acc = g2_double(acc);
        if ((s_canon.v[b >> 5] >> (b & 31)) & 1) {
            acc = started ? g2_add(acc, p) : p;
            started = true;
        }
    }
    return acc;
}
EZ_D g2a_t ld_g2a(const g2a_t* p) {
    g2a_t r;
    r.x.a = ld_fe(&p->x.a); r.x.b = ld_fe(&p->x.b); r.y.a = ld_fe(&p->y.a); r.y.b = ld_fe(&p->y.b);
    return r;
}

// thread t: sum over i = t, t + T, ... of scalars[i] * points[i]  ->  partial[t] (Jacobian)
__global__ __launch_bounds__(64) void g2_msm_partial_kernel(const g2a_t* pts, const fe_t* scalars, size_t n, g2j_t* partial, uint32_t T) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    g2j_t acc = g2_identity();
    for (size_t i = t; i < n; i += T) {
        const fe_t s = Fr::from_mont(ld_fe(scalars + i));
        acc = g2_add(acc, g2_scalar_mul(g2_from_affine(ld_g2a(pts + i)), s));
    }
    partial[t] = acc;
}
// one workgroup folds the T <= 1024 partial sums (strided per thread, then an LDS tree) and normalises
__global__ __launch_bounds__(64) void g2_msm_reduce_kernel(const g2j_t* partial, uint32_t T, g2a_t* out) {
    __shared__ g2j_t sh[64];
    g2j_t acc = g2_identity();
    for (uint32_t i = threadIdx.x; i < T; i += 64) acc = g2_add(acc, partial[i]);
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (uint32_t s = 32; s > 0; s >>= 1) {
        if (threadIdx.x < s) sh[threadIdx.x] = g2_add(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = g2_to_affine(sh[0]);
}

// ---- the bucket chain --------------------------------------------------------------------------------------------------------------
// XYZZ (extended Jacobian): x = X / ZZ, y = Y / ZZZ, ZZ^3 = ZZZ^2; identity: ZZ = 0 whatever the rest holds.  8 Fq values, 256 bytes.
struct g2x_t {
    fq2_t x, y, zz, zzz;
};
static_assert(sizeof(g2x_t) == MSM_G2_POINT_BYTES, "msm_plan_g2 lays the scratch out in points of this size");
EZ_D g2x_t g2x_identity() { return g2x_t{f2_zero(), f2_zero(), f2_zero(), f2_zero()}; }
EZ_D bool g2x_is_id(const g2x_t& p) { return f2_is_zero(p.zz); }
EZ_D fq2_t ld_f2(const fq2_t* p) { return fq2_t{ld_fe(&p->a), ld_fe(&p->b)}; }
EZ_D void st_f2(fq2_t* p, const fq2_t& v) { st_fe(&p->a, v.a); st_fe(&p->b, v.b); }
EZ_D g2x_t ld_g2x(const g2x_t* p) { return g2x_t{ld_f2(&p->x), ld_f2(&p->y), ld_f2(&p->zz), ld_f2(&p->zzz)}; }
EZ_D void st_g2x(g2x_t* p, const g2x_t& v) { st_f2(&p->x, v.x); st_f2(&p->y, v.y); st_f2(&p->zz, v.zz); st_f2(&p->zzz, v.zzz); }
// the tail of a doubling, shared by the affine and the XYZZ form: U = 2Y, V = U^2, W = U V, S = X V, M = 3 X^2 (a = 0)
EZ_D g2x_t g2x_double_core(const fq2_t& X, const fq2_t& Y, fq2_t& V, fq2_t& W) {
    const fq2_t U = f2_dbl(Y);
    V = f2_sqr(U);
    W = f2_mul(U, V);
    const fq2_t S = f2_mul(X, V), X2 = f2_sqr(X), M = f2_add(f2_dbl(X2), X2);
    g2x_t r;
    r.x = f2_sub(f2_sqr(M), f2_dbl(S));
    r.y = f2_sub(f2_mul(M, f2_sub(S, r.x)), f2_mul(W, Y));
    return r;
}
EZ_D g2x_t g2x_double_affine(const fq2_t& x, const fq2_t& y) {         // mdbl-2008-s-1; y = 0 gives ZZ = 0, the identity, as it must
    fq2_t V, W;
    g2x_t r = g2x_double_core(x, y, V, W);
    r.zz = V; r.zzz = W;
    return r;
}
EZ_D g2x_t g2x_double(const g2x_t& p) {                                // dbl-2008-s-1; the identity stays the identity (ZZ3 = V * 0)
    fq2_t V, W;
    g2x_t r = g2x_double_core(p.x, p.y, V, W);
    r.zz = f2_mul(V, p.zz); r.zzz = f2_mul(W, p.zzz);
    return r;
}
// the common tail of both additions: P = U2 - U1 != 0, R = S2 - S1; the caller multiplies ZZ, ZZZ by PP, PPP
EZ_D g2x_t g2x_add_core(const fq2_t& U1, const fq2_t& S1, const fq2_t& P, const fq2_t& R, fq2_t& PP, fq2_t& PPP) {
    PP = f2_sqr(P);
    PPP = f2_mul(P, PP);
    const fq2_t Q = f2_mul(U1, PP);
    g2x_t r;
    r.x = f2_sub(f2_sub(f2_sqr(R), PPP), f2_dbl(Q));
    r.y = f2_sub(f2_mul(R, f2_sub(Q, r.x)), f2_mul(S1, PPP));
    return r;
}
// madd-2008-s with every edge: the identity record (0, 0), an identity accumulator, P + P (a doubling) and P + (-P) (the identity).
// neg: add -q.  8 M + 2 S over Fq2 = 28 Fq products on the common path.
EZ_D g2x_t g2x_add_mixed(const g2x_t& p, const g2a_t& q, bool neg) {
    if (f2_is_zero(q.x) && f2_is_zero(q.y)) return p;
    const fq2_t qy = neg ? f2_neg(q.y) : q.y;
    if (g2x_is_id(p)) return g2x_t{q.x, qy, f2_one(), f2_one()};
    const fq2_t P = f2_sub(f2_mul(q.x, p.zz), p.x), R = f2_sub(f2_mul(qy, p.zzz), p.y);
    if (f2_is_zero(P)) return f2_is_zero(R) ? g2x_double_affine(q.x, qy) : g2x_identity();
    fq2_t PP, PPP;
    g2x_t r = g2x_add_core(p.x, p.y, P, R, PP, PPP);
    r.zz = f2_mul(p.zz, PP); r.zzz = f2_mul(p.zzz, PPP);
    return r;
}
// add-2008-s with the same edges: 12 M + 2 S over Fq2 = 40 Fq products
EZ_D g2x_t g2x_add(const g2x_t& p, const g2x_t& q) {
    if (g2x_is_id(p)) return q;
    if (g2x_is_id(q)) return p;
    const fq2_t U1 = f2_mul(p.x, q.zz), S1 = f2_mul(p.y, q.zzz);
    const fq2_t P = f2_sub(f2_mul(q.x, p.zz), U1), R = f2_sub(f2_mul(q.y, p.zzz), S1);
    if (f2_is_zero(P)) return f2_is_zero(R) ? g2x_double(p) : g2x_identity();
    fq2_t PP, PPP;
    g2x_t r = g2x_add_core(U1, S1, P, R, PP, PPP);
    r.zz = f2_mul(f2_mul(p.zz, q.zz), PP); r.zzz = f2_mul(f2_mul(p.zzz, q.zzz), PPP);
    return r;
}
// k * p for a small k (a lane's or a segment's first weight: below 2^10), from the top bit; k = 0: the identity
EZ_D g2x_t g2x_mul_small(const g2x_t& p, uint32_t k) {
    g2x_t acc = g2x_identity();
#pragma unroll 1
    for (int b = 31 - __clz(k | 1u); b >= 0; b--) {
        acc = g2x_double(acc);
        if ((k >> b) & 1u) acc = g2x_add(acc, p);
    }
    return acc;
}
// sh[0] = sum of sh[0 .. T) (T a power of two, one entry per thread), every thread of the workgroup calls it
EZ_D void g2x_lds_tree(g2x_t* sh, uint32_t T) {
    __syncthreads();
#pragma unroll 1
    for (uint32_t s = T >> 1; s > 0; s >>= 1) {
        if (threadIdx.x < s) sh[threadIdx.x] = g2x_add(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
}
template <class T> EZ_D T* g2_shift(T* p, size_t bytes) { return reinterpret_cast<T*>(reinterpret_cast<char*>(p) + bytes); }
template <class T> EZ_D const T* g2_shift(const T* p, size_t bytes) { return reinterpret_cast<const T*>(reinterpret_cast<const char*>(p) + bytes); }

// A pair of the sorted lists: the point's index and the sign of its digit.  The 128-byte record is eight 16-byte global loads.
EZ_D g2a_t g2_fetch(const g2a_t* pts, uint32_t v) { return ld_g2a(pts + (v & 0x7fffffffu)); }
// accumulate: member blockIdx.z of the group is one window; LANE = BUCKET.  A lane walks its bucket's run of the sorted payloads
// [offsets[b], offsets[b + 1]) with the next payload and the next record loaded one addition ahead (the eight loads are in flight
// under the ~28 dependent products of the addition that precedes their use).  Whole runs per lane: with at most 2^10 buckets per window and
// up to 16 windows in a launch, the lanes of a launch are fewer than the device holds at one wave per SIMD, so a balanced split of the pairs
// (the G1 kernel's lanes and fix-ups) would buy nothing here.  What breaks lane = bucket is skew, and a run longer than long_run is not walked:
// the lane queues its bucket for g2_accumulate_long_kernel.  One-wave workgroups spread the few waves over the CUs.
__global__ __launch_bounds__(64) void g2_accumulate_kernel(const g2a_t* pts, const uint32_t* offsets, const uint32_t* vals, uint32_t* long_list,
                                                           uint32_t* long_count, size_t bstride, uint32_t nb, uint32_t long_run, g2x_t* buckets) {
    const size_t bo = (size_t)blockIdx.z * bstride;
    offsets = g2_shift(offsets, bo); vals = g2_shift(vals, bo); long_list = g2_shift(long_list, bo); long_count = g2_shift(long_count, bo);
    buckets += (size_t)blockIdx.z * nb;
    const uint32_t b = blockIdx.x * 64 + threadIdx.x;
    if (b >= nb) return;
    const uint32_t beg = offsets[b], end = offsets[b + 1];
    if (end - beg > long_run) {
        long_list[atomicAdd(long_count, 1u)] = b;
        return;
    }
    g2x_t acc = g2x_identity();
    if (beg < end) {
        uint32_t v = vals[beg];
        g2a_t nxt = g2_fetch(pts, v);
#pragma unroll 1
        for (uint32_t k = beg; k < end; k++) {
            const g2a_t cur = nxt;
            const bool neg = (v >> 31) != 0;
            if (k + 1 < end) {
                v = vals[k + 1];
                nxt = g2_fetch(pts, v);
            }
            acc = g2x_add_mixed(acc, cur, neg);
        }
    }
    st_g2x(buckets + b, acc);
}
// the long runs (a column of equal scalars puts all n pairs of a window into one bucket): a workgroup per queued bucket, every thread a
// strided share of the run, the MSM_G2_LONG_THREADS partial sums folded by a tree through LDS (32 KiB)
__global__ __launch_bounds__(MSM_G2_LONG_THREADS) void g2_accumulate_long_kernel(const g2a_t* pts, const uint32_t* offsets, const uint32_t* vals,
                                                                                 const uint32_t* long_list, const uint32_t* long_count, size_t bstride,
                                                                                 uint32_t nb, g2x_t* buckets) {
    __shared__ g2x_t sh[MSM_G2_LONG_THREADS];
    const size_t bo = (size_t)blockIdx.z * bstride;
    offsets = g2_shift(offsets, bo); vals = g2_shift(vals, bo); long_list = g2_shift(long_list, bo); long_count = g2_shift(long_count, bo);
    buckets += (size_t)blockIdx.z * nb;
    const uint32_t count = *long_count < nb ? *long_count : nb;
#pragma unroll 1
    for (uint32_t h = blockIdx.x; h < count; h += gridDim.x) {
        const uint32_t b = long_list[h], beg = offsets[b], end = offsets[b + 1];
        g2x_t acc = g2x_identity();
        uint32_t k = beg + threadIdx.x;
        if (k < end) {
            uint32_t v = vals[k];
            g2a_t nxt = g2_fetch(pts, v);
#pragma unroll 1
            for (; k < end; k += MSM_G2_LONG_THREADS) {
                const g2a_t cur = nxt;
                const bool neg = (v >> 31) != 0;
                if (k + MSM_G2_LONG_THREADS < end) {
                    v = vals[k + MSM_G2_LONG_THREADS];
                    nxt = g2_fetch(pts, v);
                }
                acc = g2x_add_mixed(acc, cur, neg);
            }
        }
        sh[threadIdx.x] = acc;
        g2x_lds_tree(sh, MSM_G2_LONG_THREADS);
        if (threadIdx.x == 0) st_g2x(buckets + b, sh[0]);
        __syncthreads();
    }
}
// reduce, first launch: sum_b (b + 1) * B_b over one SEGMENT of MSM_G2_SEG buckets per workgroup (one wave), as (C, T): C the weighted sum
// with the segment's first bucket at weight 1, T the plain sum.  Lane l scans its MSM_G2_LANE_K consecutive buckets from the top with a
// running suffix sum (run += B; U += run: two additions per bucket, U = sum_j (j + 1) B_j), lifts U by its own first weight
// (U + (l K) * run, a double-and-add of at most 8 bits) and the 64 lane results of both kinds are folded by trees through LDS (32 KiB).
__global__ __launch_bounds__(64) void g2_reduce_seg_kernel(const g2x_t* buckets, uint32_t nb, uint32_t nseg, g2x_t* seg) {
    __shared__ g2x_t shC[64], shT[64];
    buckets += (size_t)blockIdx.z * nb;
    seg += ((size_t)blockIdx.z * nseg + blockIdx.x) * 2;
    const uint32_t l = threadIdx.x, base = blockIdx.x * MSM_G2_SEG + l * MSM_G2_LANE_K;
    g2x_t run = g2x_identity(), U = g2x_identity();
#pragma unroll 1
    for (uint32_t j = MSM_G2_LANE_K; j-- > 0;) {
        if (base + j < nb) run = g2x_add(run, ld_g2x(buckets + base + j));
        U = g2x_add(U, run);
    }
    shC[l] = g2x_add(U, g2x_mul_small(run, l * MSM_G2_LANE_K));
    shT[l] = run;
    __syncthreads();
#pragma unroll 1
    for (uint32_t s = 32; s > 0; s >>= 1) {
        if (l < s) {
            shC[l] = g2x_add(shC[l], shC[l + s]);
            shT[l] = g2x_add(shT[l], shT[l + s]);
        }
        __syncthreads();
    }
    if (l == 0) { st_g2x(seg, shC[0]); st_g2x(seg + 1, shT[0]); }
}
// reduce, second launch: a workgroup per window combines the segments, S_w = sum_s C_s + (s * MSM_G2_SEG) * T_s
__global__ __launch_bounds__(64) void g2_reduce_win_kernel(const g2x_t* seg, uint32_t nseg, g2x_t* win) {
    __shared__ g2x_t sh[64];
    seg += (size_t)blockIdx.z * nseg * 2;
    g2x_t acc = g2x_identity();
#pragma unroll 1
    for (uint32_t s = threadIdx.x; s < nseg; s += 64) {
        acc = g2x_add(acc, ld_g2x(seg + 2 * s));
        acc = g2x_add(acc, g2x_mul_small(ld_g2x(seg + 2 * s + 1), s * MSM_G2_SEG));
    }
    sh[threadIdx.x] = acc;
    g2x_lds_tree(sh, 64);
    if (threadIdx.x == 0) st_g2x(win + blockIdx.z, sh[0]);
}
// tail: acc = S_{W-1}, then acc = 2^width(w) * acc + S_w for w = W-2 .. 0, and the canonical affine form (one f2_inv) -- 254 dependent
// doublings, so one lane, in Jacobian coordinates (a doubling is 16 Fq products there against 24 in XYZZ).  (X, Y, ZZ, ZZZ) is the
// Jacobian point (X ZZ, Y ZZZ, ZZ): Z^2 = ZZ^2 and Z^3 = ZZ^3 = ZZZ^2.
__global__ __launch_bounds__(64) void g2_tail_kernel(const g2x_t* win, WinPlan wp, g2a_t* out) {
    if (threadIdx.x) return;
    g2j_t acc = g2_identity();
#pragma unroll 1
    for (uint32_t w = wp.W; w-- > 0;) {
        if (w + 1 < wp.W) {
#pragma unroll 1
            for (uint32_t k = 0; k < wp.width(w); k++) acc = g2_double(acc);
        }
        const g2x_t s = ld_g2x(win + w);
        if (!g2x_is_id(s)) acc = g2_add(acc, g2j_t{f2_mul(s.x, s.zz), f2_mul(s.y, s.zzz), s.zz});
    }
    const g2a_t r = g2_to_affine(acc);
    st_f2(&out->x, r.x); st_f2(&out->y, r.y);
}

// points: n resident 128-byte affine records, scalars: n resident Montgomery Fr; out_host: 128 bytes; returns after `st` has drained
int g2_msm_points_run(Ctx* c, hipStream_t st, const void* pts_dev, const fe_t* scalars_dev, size_t n, void* out_host) {
    if (n == 0) return EZKL_ERR_INVALID;
    if (n >= ((size_t)1 << 31)) return EZKL_ERR_UNSUPPORTED;      // a payload is 31 bits of index and the sign
    MsmG2Plan q;
    uint8_t* base = nullptr;
    int rc = msm_g2_prepare(c, n, &q, &base);
    if (rc) return rc;
    const MsmPlan& p = q.chain;
    if (p.LB != 0 || p.nb != q.nb) return EZKL_ERR_UNSUPPORTED;   // the reduce kernels weigh position b as bucket b (msm_plan_g2)
    const g2a_t* pts = (const g2a_t*)pts_dev;
    uint8_t* S = base + q.o_slabs;
    g2x_t *bkt = (g2x_t*)(base + q.o_bkt), *seg = (g2x_t*)(base + q.o_seg), *win = (g2x_t*)(base + q.o_win);
    g2a_t* d_out = (g2a_t*)(base + q.o_out);
    const uint32_t *offs = (const uint32_t*)(S + p.o.offs), *vals = (const uint32_t*)(S + p.o.vals);
    uint32_t *long_list = (uint32_t*)(S + p.o.heavy), *long_count = (uint32_t*)(S + p.o.hcnt);     // zeroed by the front end's first kernel
    hipEvent_t m0 = nullptr, m1 = nullptr;
    if ((rc = ev_pair(c, "msm_g2", &m0, &m1))) return rc;
    EZ_HIP(hipEventRecord(m0, st));
    for (size_t g = 0; g < q.ngroups; g++) {                      // one sequence of launches per group of windows; the groups reuse the slabs
        const uint32_t w0 = (uint32_t)(g * q.group);
        const unsigned Z = (unsigned)(q.wp.W - w0 < q.group ? q.wp.W - w0 : q.group);
        msm_once_sort_enqueue(st, scalars_dev, n, q.wp, p, w0, Z, S);
        hipLaunchKernelGGL(g2_accumulate_kernel, dim3(cdiv(q.nb, 64), 1, Z), dim3(64), 0, st, pts, offs, vals, long_list, long_count, p.bstride, q.nb,
                           q.long_run, bkt);
        hipLaunchKernelGGL(g2_accumulate_long_kernel, dim3(q.long_blocks, 1, Z), dim3(MSM_G2_LONG_THREADS), 0, st, pts, offs, vals,
                           (const uint32_t*)long_list, (const uint32_t*)long_count, p.bstride, q.nb, bkt);
        hipLaunchKernelGGL(g2_reduce_seg_kernel, dim3(q.nseg, 1, Z), dim3(64), 0, st, (const g2x_t*)bkt, q.nb, q.nseg, seg);
        hipLaunchKernelGGL(g2_reduce_win_kernel, dim3(1, 1, Z), dim3(64), 0, st, (const g2x_t*)seg, q.nseg, win + w0);
    }
    hipLaunchKernelGGL(g2_tail_kernel, dim3(1), dim3(64), 0, st, (const g2x_t*)win, q.wp, d_out);
    EZ_HIP(hipGetLastError());
    EZ_HIP(hipEventRecord(m1, st));
    EZ_HIP(hipMemcpyAsync(out_host, d_out, sizeof(g2a_t), hipMemcpyDeviceToHost, st));
    EZ_HIP(hipStreamSynchronize(st));
    return EZKL_OK;
}

// ---- is every record of a resident set a point of G2?  (DESIGN.md §4.1 "G2 set check") ------------------------------------------------
// The twist's group E'(Fq2) has order r (2q - r): a record can be canonical and on the curve and still have an order other than r, and a
// sum or a pairing over it means nothing.  Per record, the first that applies:
//   1  one of the four coordinate words >= q        2  y^2 != x^3 + 3 / xi        3  on the twist, not of order r
// and the all-zero record is the identity: valid, counted apart (what g2x_add_mixed skips).  The order test is not [r]P: with
// psi = twist . Frobenius . untwist, psi(x, y) = (conj(x) xi^((q-1)/3), conj(y) xi^((q-1)/2)), and the BN parameter x,
//     [x + 1]P + psi([x]P) + psi^2([x]P) == psi^3([2x]P)
// holds exactly for the points of order r (DESIGN.md says why).  ONE 63-bit product A = [x]P; the rest is Horner in psi,
//     T = psi(A + psi(A - psi(2A))) = psi(A) + psi^2(A) - psi^3(2A),        L = A + P,        valid  <=>  L == -T,
// three maps, a doubling and three additions, the comparison cross-multiplied (no inversion).  psi acts on XYZZ coordinate by coordinate
// (conjugation is a field automorphism, so ZZ^3 = ZZZ^2 survives): two constant products, and the two constants come from
// tools/gen_constants.py like the twist's b.  x is a constant: its signed digits (non-adjacent form, read off 3x and x: 24 non-zero ones
// against 28 set bits) steer one loop whose branches are uniform, 62 doublings and 23 mixed additions of +-P, the same for every lane.
struct G2Const {
    static constexpr uint32_t B0[8] = BN32_FQ2_TWIST_B_C0_INIT, B1[8] = BN32_FQ2_TWIST_B_C1_INIT;
    static constexpr uint32_t PX0[8] = BN32_FQ2_PSI_X_C0_INIT, PX1[8] = BN32_FQ2_PSI_X_C1_INIT;
    static constexpr uint32_t PY0[8] = BN32_FQ2_PSI_Y_C0_INIT, PY1[8] = BN32_FQ2_PSI_Y_C1_INIT;
};
constexpr uint64_t BN_X = 4965661367192848881ull;
constexpr uint64_t BN_X_POS = ((3 * BN_X) & ~BN_X) >> 1, BN_X_NEG = (~(3 * BN_X) & BN_X) >> 1;     // digit b of x is +1 / -1 where bit b is set
static_assert(BN_X < (1ull << 63) / 3 * 2 && BN_X_POS - BN_X_NEG == BN_X && (BN_X_POS >> 62) == 1, "3x fits 64 bits; the top digit is +1 at 2^62");
enum : uint32_t { G2_OK = 0, G2_NOT_CANONICAL = 1, G2_OFF_CURVE = 2, G2_OFF_SUBGROUP = 3 };

EZ_D fq2_t f2_const(const uint32_t (&c0)[8], const uint32_t (&c1)[8]) { return fq2_t{fr_const(c0), fr_const(c1)}; }
EZ_D bool f2_eq(const fq2_t& x, const fq2_t& y) { return Fq::eq(x.a, y.a) && Fq::eq(x.b, y.b); }
EZ_D fq2_t f2_conj(const fq2_t& x) { return fq2_t{x.a, Fq::neg(x.b)}; }
EZ_D g2x_t g2x_psi(const g2x_t& p) {
    return g2x_t{f2_mul(f2_conj(p.x), f2_const(G2Const::PX0, G2Const::PX1)), f2_mul(f2_conj(p.y), f2_const(G2Const::PY0, G2Const::PY1)),
                 f2_conj(p.zz), f2_conj(p.zzz)};
}
EZ_D bool fe_ge_q(const fe_t& a) {                                       // a >= q as 256-bit integers: a - q leaves no borrow
    uint32_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) (void)subb32(a.v[i], FqP::MOD[i], br);
    return br == 0;
}
// p is on the twist and not the identity: is it of order r?
EZ_D bool g2_has_order_r(const g2a_t& p) {
    g2x_t A{p.x, p.y, f2_one(), f2_one()};
#pragma unroll 1
    for (int b = 61; b >= 0; b--) {
        A = g2x_double(A);
        if (((BN_X_POS | BN_X_NEG) >> b) & 1) A = g2x_add_mixed(A, p, (BN_X_NEG >> b) & 1);
    }
    g2x_t T = g2x_psi(g2x_double(A));
    T.y = f2_neg(T.y);
    T = g2x_psi(g2x_add(A, T));
    T = g2x_psi(g2x_add(A, T));
    const g2x_t L = g2x_add_mixed(A, p, false);
    if (g2x_is_id(L) || g2x_is_id(T)) return g2x_is_id(L) && g2x_is_id(T);
    return f2_eq(f2_mul(L.x, T.zz), f2_mul(T.x, L.zz)) && f2_eq(f2_mul(L.y, T.zzz), f2_neg(f2_mul(T.y, L.zzz)));
}
EZ_D uint32_t g2_point_reason(const g2a_t& p, bool* identity) {
    *identity = f2_is_zero(p.x) && f2_is_zero(p.y);
    if (*identity) return G2_OK;
    if (fe_ge_q(p.x.a) || fe_ge_q(p.x.b) || fe_ge_q(p.y.a) || fe_ge_q(p.y.b)) return G2_NOT_CANONICAL;
    const fq2_t rhs = f2_add(f2_mul(f2_sqr(p.x), p.x), f2_const(G2Const::B0, G2Const::B1));
    if (!f2_eq(f2_sqr(p.y), rhs)) return G2_OFF_CURVE;
    return g2_has_order_r(p) ? G2_OK : G2_OFF_SUBGROUP;
}
// One lane per point in XYZZ, G2_CHECK_THREADS lanes a workgroup, at most one workgroup per CU, each lane striding over the set with its
// next record's eight loads issued before this record's ~2 200 products.  ONE wave per SIMD: the accumulator, the record, the next record
// and the temporaries of an XYZZ + XYZZ addition over Fq2 take 256 VGPRs and 64 AGPRs and no scratch; held to the 168 registers of three
// waves per SIMD the compiler moves 892 registers through 1 280 bytes of scratch per lane.  The outputs are g1_check_kernel's:
// acc[0] += bad points, acc[1] = min over bad points of (index << 2 | reason), acc[2] += identities -- two sums and a minimum, so the answer
// does not depend on the order the waves arrive in; counts are wave ballots (a lane that has left the loop votes 0), a wave touches memory
// only if it has something to report, with vector atomics.  Any bytes are legal input: the predicate branches on them, never indexes by them.
constexpr unsigned G2_CHECK_THREADS = 256;
__global__ __launch_bounds__(G2_CHECK_THREADS) void g2_check_kernel(const g2a_t* pts, size_t n, unsigned long long* acc) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long key = ~0ull;
    uint32_t n_bad = 0, n_id = 0;
    g2a_t next;
    if (i < n) next = ld_g2a(pts + i);
    while (i < n) {
        const g2a_t p = next;
        if (i + stride < n) next = ld_g2a(pts + i + stride);
        bool id;
        const uint32_t reason = g2_point_reason(p, &id);
        n_bad += reason != 0;
        n_id += id;
        if (reason) {
            const unsigned long long k = ((unsigned long long)i << 2) | reason;
            key = k < key ? k : key;
        }
        i += stride;
    }
    // lanes leave the loop at different trips, so the counts are per lane and summed across the wave here
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const unsigned long long o = __shfl_xor(key, off);
        key = o < key ? o : key;
        n_bad += __shfl_xor(n_bad, off);
        n_id += __shfl_xor(n_id, off);
    }
    if ((threadIdx.x & 63) == 0) {
        if (n_bad) {
            atomicAdd(acc, (unsigned long long)n_bad);
            atomicMin(acc + 1, key);
        }
        if (n_id) atomicAdd(acc + 2, (unsigned long long)n_id);
    }
}
// out: {bad points, smallest bad index or UINT64_MAX, its reason, identities}; returns after `st` has drained
int g2_check(Ctx* c, hipStream_t st, const void* pts_dev, size_t n, uint64_t out[4]) {
    out[0] = 0; out[1] = UINT64_MAX; out[2] = 0; out[3] = 0;
    if (n == 0) return EZKL_ERR_INVALID;
    unsigned long long* acc = nullptr;
    int rc = arena_reserve(c->aux, 32, st, (void**)&acc);
    if (rc) return rc;
    hipEvent_t e0, e1;
    if ((rc = ev_pair(c, "g2_check", &e0, &e1))) return rc;
    EZ_HIP(hipMemsetAsync(acc, 0, 32, st));
    EZ_HIP(hipMemsetAsync(acc + 1, 0xff, 8, st));
    const unsigned blocks = std::min<size_t>(cdiv(n, G2_CHECK_THREADS), (size_t)std::max(c->num_cus, 1));
    EZ_HIP(hipEventRecord(e0, st));
    hipLaunchKernelGGL(g2_check_kernel, dim3(blocks), dim3(G2_CHECK_THREADS), 0, st, (const g2a_t*)pts_dev, n, acc);
    EZ_HIP(hipGetLastError());
    EZ_HIP(hipEventRecord(e1, st));
    unsigned long long host[3] = {0, 0, 0};
    EZ_HIP(hipMemcpyAsync(host, acc, sizeof host, hipMemcpyDeviceToHost, st));
    if ((rc = arena_done(c->aux, st))) return rc;
    EZ_HIP(hipStreamSynchronize(st));
    out[0] = host[0];
    out[3] = host[2];
    if (host[1] != ~0ull) { out[1] = host[1] >> 2; out[2] = host[1] & 3; }
    return EZKL_OK;
}

int g2_msm(Ctx* c, hipStream_t st, const void* pts_host, const void* scalars_host, size_t n, void* out_host) {
    if (n == 0) { memset(out_host, 0, 128); return EZKL_OK; }
    g2a_t *d_pts = nullptr, *d_out = nullptr;
    fe_t* d_sc = nullptr;
    g2j_t* d_part = nullptr;
    const uint32_t T = (uint32_t)(n < 1024 ? n : 1024);
    int rc = EZKL_OK;
    hipError_t e = hipMalloc(&d_pts, n * sizeof(g2a_t));
    if (e == hipSuccess) e = hipMalloc(&d_sc, n * sizeof(fe_t));
    if (e == hipSuccess) e = hipMalloc(&d_part, (size_t)T * sizeof(g2j_t));
    if (e == hipSuccess) e = hipMalloc(&d_out, sizeof(g2a_t));
    if (e == hipSuccess) e = hipMemcpyAsync(d_pts, pts_host, n * sizeof(g2a_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_sc, scalars_host, n * sizeof(fe_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && n >= MSM_G2_CROSSOVER) {          // the bucket chain on the uploaded copies
        rc = g2_msm_points_run(c, st, d_pts, d_sc, n, out_host);
    } else if (e == hipSuccess) {
        hipLaunchKernelGGL(g2_msm_partial_kernel, dim3(cdiv(T, 64)), dim3(64), 0, st, (const g2a_t*)d_pts, (const fe_t*)d_sc, n, d_part, T);
        hipLaunchKernelGGL(g2_msm_reduce_kernel, dim3(1), dim3(64), 0, st, (const g2j_t*)d_part, T, d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess && n < MSM_G2_CROSSOVER) e = hipMemcpyAsync(out_host, d_out, sizeof(g2a_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) rc = set_hip_error(e, "g2_msm", __FILE__, __LINE__);
    if (d_pts) (void)hipFree(d_pts);
    if (d_sc) (void)hipFree(d_sc);
    if (d_part) (void)hipFree(d_part);
    if (d_out) (void)hipFree(d_out);
    return rc;
}

}  // namespace ezkl
