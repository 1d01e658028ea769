// fieldprobe.hip -- test-only: ONE field primitive of field.hpp / field29.hpp applied to n rows of operands (ezkl_hip_field_probe_dev).
//
// The suite reaches the two field layers almost only through whole kernels on random residues; this entry point lets a test put a
// chosen word (a limb of 0 or 0xffffffff, a value on p, 2p or K p) into one primitive and read back exactly what the device computed.
// Every primitive is a kernel of its own (the primitive is a template argument, the host dispatches from one table by name): a single
// kernel with a run-time switch would keep every operand live around every product and exercise none of them the way production does.
// One lane per row, grid-stride, 256 threads.  Rows are uint32 words: 8 per element in radix 2^32, 9 in radix 2^29, 1 for a flag.
//
// The "live" probes wrap one inline-assembly product in LIVE_ROWS further operand rows (vector registers) and LIVE_SALT uniform words
// (scalar registers) that are alive across it, and write product, rows and words back: the assembly names v16..v28 and s16..s26 in its
// text, and only its clobber list keeps the register allocator from parking a value there.
#include <string.h>
#include "common.hpp"
#include "field29.hpp"

namespace ezkl {
namespace {

typedef void (*probe_kernel_t)(const uint32_t*, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t*, size_t);

template <class Op>
__global__ __launch_bounds__(256) void probe_kernel(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, const uint32_t* __restrict__ c,
                                                    const uint32_t* __restrict__ d, uint32_t* __restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) Op::run(a, b, c, d, out, i, n);
}

EZ_D fe_t ld8(const uint32_t* p, size_t i) { return ld_fe(reinterpret_cast<const fe_t*>(p) + i); }
EZ_D void st8(uint32_t* p, size_t i, const fe_t& x) { st_fe(reinterpret_cast<fe_t*>(p) + i, x); }
EZ_D f29_t ld9(const uint32_t* p, size_t i) { return ld_f29(reinterpret_cast<const f29_t*>(p) + i); }
EZ_D void st9(uint32_t* p, size_t i, const f29_t& x) { st_f29(reinterpret_cast<f29_t*>(p) + i, x); }

#define PROBE_ARGS const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out, size_t i, size_t n

// ---- radix 2^32: F = Field<FrP> or Field<FqP> ----
#define OP32_1(NAME, EXPR)                                                             \
    template <class F> struct NAME {                                                   \
        static constexpr int ARITY = 1, IN = 8, OUT = 8;                               \
        EZ_D static void run(PROBE_ARGS) { const fe_t x = ld8(a, i); st8(out, i, EXPR); } \
    }
#define OP32_2(NAME, EXPR)                                                             \
    template <class F> struct NAME {                                                   \
        static constexpr int ARITY = 2, IN = 8, OUT = 8;                               \
        EZ_D static void run(PROBE_ARGS) { const fe_t x = ld8(a, i), y = ld8(b, i); st8(out, i, EXPR); } \
    }
OP32_2(P_add, F::add(x, y));
OP32_2(P_sub, F::sub(x, y));
OP32_1(P_neg, F::neg(x));
OP32_1(P_dbl, F::dbl(x));
OP32_1(P_reduce_once, F::reduce_once(x));
OP32_2(P_mul, F::mul(x, y));
OP32_2(P_mul_inl, F::mul_inl(x, y));
OP32_1(P_sqr, F::sqr(x));
OP32_2(P_mul_lazy, F::mul_lazy(x, y));
OP32_1(P_redc, F::redc(x));
OP32_1(P_from_mont, F::from_mont(x));
OP32_1(P_to_mont, F::to_mont(x));
OP32_2(P_add_lazy, F::add_lazy(x, y));
OP32_2(P_sub_lazy, F::sub_lazy(x, y));
OP32_1(P_reduce_2p, F::reduce_2p(x));
OP32_1(P_inv, F::inv(x));

// ---- radix 2^29: F = Fr29 or Fq29 ----
#define OP29_1(NAME, EXPR)                                                             \
    template <class F> struct NAME {                                                   \
        static constexpr int ARITY = 1, IN = 9, OUT = 9;                               \
        EZ_D static void run(PROBE_ARGS) { const f29_t x = ld9(a, i); st9(out, i, EXPR); } \
    }
#define OP29_1K(NAME, EXPR)                                                            \
    template <class F, int KI> struct NAME {                                           \
        static constexpr int ARITY = 1, IN = 9, OUT = 9;                               \
        EZ_D static void run(PROBE_ARGS) { const f29_t x = ld9(a, i); st9(out, i, EXPR); } \
    }
#define OP29_2(NAME, EXPR)                                                             \
    template <class F> struct NAME {                                                   \
        static constexpr int ARITY = 2, IN = 9, OUT = 9;                               \
        EZ_D static void run(PROBE_ARGS) { const f29_t x = ld9(a, i), y = ld9(b, i); st9(out, i, EXPR); } \
    }
template <class F> struct Q_unpack {
    static constexpr int ARITY = 1, IN = 8, OUT = 9;
    EZ_D static void run(PROBE_ARGS) { st9(out, i, F::unpack(ld8(a, i))); }
};
template <class F> struct Q_pack {
    static constexpr int ARITY = 1, IN = 9, OUT = 8;
    EZ_D static void run(PROBE_ARGS) { st8(out, i, F::pack(ld9(a, i))); }
};
OP29_1(Q_normalize, F::normalize(x));
OP29_2(Q_mul, F::mul(x, y));
OP29_2(Q_mul_cold, F::mul_cold(x, y));
OP29_1(Q_sqr, F::sqr(x));
OP29_1(Q_sqr_cold, F::sqr_cold(x));
template <class F> struct Q_mul2add {
    static constexpr int ARITY = 4, IN = 9, OUT = 9;
    EZ_D static void run(PROBE_ARGS) { st9(out, i, F::mul2add(ld9(a, i), ld9(b, i), ld9(c, i), ld9(d, i))); }
};
template <class F, int KI> struct Q_sub {
    static constexpr int ARITY = 2, IN = 9, OUT = 9;
    EZ_D static void run(PROBE_ARGS) { st9(out, i, F::template sub<KI>(ld9(a, i), ld9(b, i))); }
};
OP29_1K(Q_neg, F::template neg<KI>(x));
OP29_1K(Q_cond_sub, F::template cond_sub<KI>(x));
OP29_1(Q_canonical, F::canonical(x));
template <class F> struct Q_is_zero_mod_p {
    static constexpr int ARITY = 1, IN = 9, OUT = 1;
    EZ_D static void run(PROBE_ARGS) { out[i] = F::is_zero_mod_p(ld9(a, i)) ? 1u : 0u; }
};

// ---- live-register probes ----
// Row i of the result: the product (W words), then rows i+1 .. i+LIVE_ROWS (mod n) of operand a as they were loaded BEFORE the product
// (LIVE_ROWS x W words), then the LIVE_SALT words live_salt(j).  A pin is an empty volatile asm statement that takes its operands in
// place: those before the product also take a word of the product's input, those after it a word of its output, so by data dependence
// the product sits between the two and every pinned value is in a register across it.
static constexpr int LIVE_ROWS = 6, LIVE_SALT = 64;
constexpr uint32_t live_salt(int j) { return 0x9e3779b9u * (uint32_t)(j + 1); }
struct LiveSalt {
    uint32_t w[LIVE_SALT];
};
__constant__ LiveSalt g_live_salt;            // filled by the host; uniform loads, so the words arrive in scalar registers

template <int W> EZ_D void pin_rows(uint32_t (&r)[LIVE_ROWS][W], uint32_t& dep) {
#pragma unroll
    for (int k = 0; k < LIVE_ROWS; k++) {
        asm volatile("" : "+v"(dep), "+v"(r[k][0]), "+v"(r[k][1]), "+v"(r[k][2]), "+v"(r[k][3]), "+v"(r[k][4]), "+v"(r[k][5]), "+v"(r[k][6]), "+v"(r[k][7]));
        if (W == 9) asm volatile("" : "+v"(dep), "+v"(r[k][W - 1]));
    }
}
EZ_D void pin_salt(uint32_t (&s)[LIVE_SALT], uint32_t& dep) {
#pragma unroll
    for (int j = 0; j < LIVE_SALT; j += 8)
        asm volatile("" : "+v"(dep), "+s"(s[j]), "+s"(s[j + 1]), "+s"(s[j + 2]), "+s"(s[j + 3]), "+s"(s[j + 4]), "+s"(s[j + 5]), "+s"(s[j + 6]), "+s"(s[j + 7]));
}
// Prod::run(x, y, z, t, r) with ARITY operands of W words each
template <class Prod>
struct LiveProbe {
    static constexpr int W = Prod::W, ARITY = Prod::ARITY, IN = W, OUT = W + LIVE_ROWS * W + LIVE_SALT;
    EZ_D static void run(PROBE_ARGS) {
        uint32_t x[W], y[W], z[W], t[W], r[W], rows[LIVE_ROWS][W], salt[LIVE_SALT];
#pragma unroll
        for (int q = 0; q < W; q++) {
            x[q] = a[i * W + q];
            y[q] = ARITY >= 2 ? b[i * W + q] : 0u;
            z[q] = ARITY == 4 ? c[i * W + q] : 0u;
            t[q] = ARITY == 4 ? d[i * W + q] : 0u;
        }
#pragma unroll
        for (int k = 0; k < LIVE_ROWS; k++) {
            const size_t row = (i + 1 + k) % n;
#pragma unroll
            for (int q = 0; q < W; q++) rows[k][q] = a[row * W + q];
        }
#pragma unroll
        for (int j = 0; j < LIVE_SALT; j++) salt[j] = g_live_salt.w[j];
        pin_rows<W>(rows, x[0]);
        pin_salt(salt, x[0]);
        Prod::run(x, y, z, t, r);
        pin_rows<W>(rows, r[0]);
        pin_salt(salt, r[0]);
        uint32_t* o = out + i * OUT;
#pragma unroll
        for (int q = 0; q < W; q++) o[q] = r[q];
#pragma unroll
        for (int k = 0; k < LIVE_ROWS; k++)
#pragma unroll
            for (int q = 0; q < W; q++) o[W + k * W + q] = rows[k][q];
#pragma unroll
        for (int j = 0; j < LIVE_SALT; j++) o[W + LIVE_ROWS * W + j] = salt[j];
    }
};
template <class P> struct L_mul_inl {              // mont_mul_asm: per-column asm statements, modulus limbs as "s" operands
    static constexpr int W = 8, ARITY = 2;
    EZ_D static void run(const uint32_t (&x)[8], const uint32_t (&y)[8], const uint32_t (&)[8], const uint32_t (&)[8], uint32_t (&r)[8]) {
        fe_t fx, fy;
#pragma unroll
        for (int q = 0; q < 8; q++) { fx.v[q] = x[q]; fy.v[q] = y[q]; }
        const fe_t o = mont_mul_asm<P>(fx, fy);
#pragma unroll
        for (int q = 0; q < 8; q++) r[q] = o.v[q];
    }
};
template <class P> struct L_mul_lazy {             // mont_mul_asm1_*: one asm statement behind the noinline call of Field::mul_lazy
    static constexpr int W = 8, ARITY = 2;
    EZ_D static void run(const uint32_t (&x)[8], const uint32_t (&y)[8], const uint32_t (&)[8], const uint32_t (&)[8], uint32_t (&r)[8]) {
        fe_t fx, fy;
#pragma unroll
        for (int q = 0; q < 8; q++) { fx.v[q] = x[q]; fy.v[q] = y[q]; }
        const fe_t o = Field<P>::mul_lazy(fx, fy);
#pragma unroll
        for (int q = 0; q < 8; q++) r[q] = o.v[q];
    }
};
template <class P> struct L_mul_single {           // mont_mul_asm1_* inlined into the probe itself: nothing but its clobber list protects the rows
    static constexpr int W = 8, ARITY = 2;
    EZ_D static void run(const uint32_t (&x)[8], const uint32_t (&y)[8], const uint32_t (&)[8], const uint32_t (&)[8], uint32_t (&r)[8]) {
        mont_mul_single<P>(x, y, r);
    }
};
template <class F> struct L_mul29 {
    static constexpr int W = 9, ARITY = 2;
    EZ_D static void run(const uint32_t (&x)[9], const uint32_t (&y)[9], const uint32_t (&)[9], const uint32_t (&)[9], uint32_t (&r)[9]) { F::mul_asm(x, y, r); }
};
template <class F> struct L_sqr29 {
    static constexpr int W = 9, ARITY = 1;
    EZ_D static void run(const uint32_t (&x)[9], const uint32_t (&)[9], const uint32_t (&)[9], const uint32_t (&)[9], uint32_t (&r)[9]) {
        f29_t fx;
#pragma unroll
        for (int q = 0; q < 9; q++) fx.v[q] = x[q];
        const f29_t o = F::sqr(fx);
#pragma unroll
        for (int q = 0; q < 9; q++) r[q] = o.v[q];
    }
};
struct L_mul2add29 {
    static constexpr int W = 9, ARITY = 4;
    EZ_D static void run(const uint32_t (&x)[9], const uint32_t (&y)[9], const uint32_t (&z)[9], const uint32_t (&t)[9], uint32_t (&r)[9]) { mont_mul2add29_fq(x, y, z, t, r); }
};

// ---- the table ----
struct Entry {
    const char* name;
    probe_kernel_t kernel;
    int arity, in_words, out_words;
};
template <class Op> constexpr Entry entry(const char* name) { return Entry{name, probe_kernel<Op>, Op::ARITY, Op::IN, Op::OUT}; }

#define E32(NAME) entry<P_##NAME<Fr>>("fr." #NAME), entry<P_##NAME<Fq>>("fq." #NAME)
#define E29(NAME) entry<Q_##NAME<Fr29>>("fr29." #NAME), entry<Q_##NAME<Fq29>>("fq29." #NAME)
#define E29K(NAME, KI) entry<Q_##NAME<Fr29, KI>>("fr29." #NAME #KI), entry<Q_##NAME<Fq29, KI>>("fq29." #NAME #KI)
const Entry TABLE[] = {
    E32(add), E32(sub), E32(neg), E32(dbl), E32(reduce_once), E32(mul), E32(mul_inl), E32(sqr), E32(mul_lazy), E32(redc), E32(from_mont), E32(to_mont),
    E32(add_lazy), E32(sub_lazy), E32(reduce_2p), E32(inv),
    E29(unpack), E29(pack), E29(normalize), E29(mul), E29(mul_cold), E29(sqr), E29(sqr_cold), entry<Q_mul2add<Fq29>>("fq29.mul2add"),
    E29K(sub, 0), E29K(sub, 1), E29K(sub, 2), E29K(sub, 3), E29K(sub, 4), E29K(sub, 5), E29K(sub, 6),
    E29K(neg, 0), E29K(neg, 1), E29K(neg, 2), E29K(neg, 3), E29K(neg, 4), E29K(neg, 5), E29K(neg, 6),
    E29K(cond_sub, 0), E29K(cond_sub, 1), E29K(cond_sub, 2), E29K(cond_sub, 3),
    E29(canonical), E29(is_zero_mod_p),
    entry<LiveProbe<L_mul_inl<FrP>>>("fr.live_mul_inl"), entry<LiveProbe<L_mul_inl<FqP>>>("fq.live_mul_inl"),
    entry<LiveProbe<L_mul_lazy<FrP>>>("fr.live_mul_lazy"), entry<LiveProbe<L_mul_lazy<FqP>>>("fq.live_mul_lazy"),
    entry<LiveProbe<L_mul_single<FrP>>>("fr.live_mul_single"), entry<LiveProbe<L_mul_single<FqP>>>("fq.live_mul_single"),
    entry<LiveProbe<L_mul29<Fr29>>>("fr29.live_mul"), entry<LiveProbe<L_mul29<Fq29>>>("fq29.live_mul"),
    entry<LiveProbe<L_sqr29<Fr29>>>("fr29.live_sqr"), entry<LiveProbe<L_sqr29<Fq29>>>("fq29.live_sqr"),
    entry<LiveProbe<L_mul2add29>>("fq29.live_mul2add"),
};
constexpr size_t TABLE_LEN = sizeof(TABLE) / sizeof(TABLE[0]);

}  // namespace

int field_probe_names(char* out, size_t cap, size_t* len) {
    std::string s;
    char line[96];
    for (size_t e = 0; e < TABLE_LEN; e++) {
        snprintf(line, sizeof line, "%s %d %d %d\n", TABLE[e].name, TABLE[e].arity, TABLE[e].in_words, TABLE[e].out_words);
        s += line;
    }
    *len = s.size();
    if (out && cap) {
        const size_t m = s.size() < cap - 1 ? s.size() : cap - 1;
        memcpy(out, s.data(), m);
        out[m] = 0;
    }
    return EZKL_OK;
}

int field_probe(Ctx* c, hipStream_t st, const char* name, const uint32_t* const ops[4], uint32_t* out, size_t n) {
    const Entry* e = nullptr;
    for (size_t k = 0; k < TABLE_LEN; k++)
        if (!strcmp(TABLE[k].name, name)) e = &TABLE[k];
    if (!e) return EZKL_ERR_INVALID;
    for (int k = 0; k < e->arity; k++)
        if (!ops[k]) return EZKL_ERR_INVALID;
    if (n == 0) return EZKL_OK;
    if (strstr(name, ".live_")) {
        LiveSalt h;
        for (int j = 0; j < LIVE_SALT; j++) h.w[j] = live_salt(j);
        EZ_HIP(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_live_salt), &h, sizeof h, 0, hipMemcpyHostToDevice, st));
        EZ_HIP(hipStreamSynchronize(st));                 // h is a stack object
    }
    const unsigned want = cdiv(n, 256), most = (unsigned)c->num_cus * 8;
    hipLaunchKernelGGL(e->kernel, dim3(want < most ? want : most), dim3(256), 0, st, ops[0], ops[1], ops[2], ops[3], out, n);
    EZ_HIP(hipGetLastError());
    return EZKL_OK;
}

}  // namespace ezkl
