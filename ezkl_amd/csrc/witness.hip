// witness.hip -- witness synthesis on the device from a recorded plan (ezkl_amd/witness_plan.py; blob layout: witness_plan.hpp).
//
// halo2 fills the advice columns in GraphCircuit::synthesize (/root/reference/src/graph/mod.rs:2010-2200) by running the model's layout
// (src/circuit/ops/layouts.rs) cell by cell on the host.  For the MLP op family which cell holds what is a function of the circuit
// alone, so the layout is recorded once as a list of RECORDS and replayed here for every proof: one launch per record into resident,
// zero-filled columns of 2^k Montgomery words.  ezkl_amd/witness_plan.py `run_plan_host` is the executable specification: a lane
// here does to one element what one iteration of its loops does.
//
//  * element-wise records (copy, const, input, param, add / sub / mult, decompose hints, range-check index, inverse-or-zero, static
//    lookup output and its table-column index, the rounded division by a constant of `div`, layouts.rs:219-267): one lane per
//    destination cell; the index arrays are read coalesced, and where they hold contiguous runs (they mostly do: the layout advances
//    a linear coordinate) so are the 32-byte cells;
//  * dot records (the running sum of w products per row, layouts.rs:532-610, with the duplicated row at the top of a new column as
//    a step without products): all dots of a record run in parallel, 16 lanes to a dot -- a chunked scan over its rows, see
//    wit_dot_kernel.  The index arrays are step-major (step s of every dot, then step s + 1): a wave holds 4 dots x 16 row chunks, so
//    one index read of a wave is 16 runs of 4 consecutive words, one run per chunk.
//
//  * the einsum family (second-phase advice: a plan with PHASES, one run per phase -- ezkl_hip_witness_run_phase_dev -- between the
//    prover's commit stages).  matmul records: the exact integer product the prover witnesses, an LDS-tiled matmul over the gathered
//    int64 inputs, see wit_matmul_kernel.  rlc records (RLCConfig::assign_rlc, /root/reference/src/circuit/ops/chip/einsum/mod.rs:785-866,
//    at block width 1: out[t] = out[t-1] * c + c * v[t]): the chunked scan of the dot records with an affine map in the combine step,
//    see wit_rlc_kernel.  The contraction "j,j->" is a dot record with w = 1; everything else is a copy.  An operand of a matmul
//    outside |v| < 2^31 is reported as the range failures below are ("einsum operand outside the exact-product range").
//
//  * the general einsum (ezkl_layout.EinsumCircuit: any two-operand equation of the Freivalds chip, over cells the circuit computed).  The
//    product the prover claims is a dot record of ONE step of K products per output element, over the operands' cells: such a record
//    (p1 == 1, p0 >= DOT_WIDE_MIN) runs on wit_dot_wide_kernel, every lane of a wave multiplying, the partial sums met by wave shuffles; the
//    lanes to a dot are chosen on the host (dot_wide_lanes).  The cells are wit_dot_kernel's bit for bit; ezkl_hip_witness_wide_dots counts
//    the launches.  The second-phase pairwise product is a mult record, the einsum's sum / prod are sum / prod records.
//
//  * the surrogate's ops.  sum / prod records (BaseRegion._accumulate, layouts.rs:2472-2621: the running sum or product of w cells per
//    row): the chunked scan of the dot records with one operand per entry and addition or the Montgomery product as the monoid, see
//    wit_acc_kernel.  gather records (row `index` of a dynamic table, the structure of `select`, layouts.rs:1483-1581): an element-wise
//    kind -- the signed index, the bounds test, then one index load and one cell copy; an index outside the table is reported as the
//    range failures below are ("gather index outside the table") and is never used as an address.  clamp records: min(max(s, lo), hi),
//    element-wise, never failing.  ezkl_hip_witness_tile_dev repeats the unit rows [0, U) a plan wrote down its columns and into the
//    columns of the other blocks, see wit_tile_kernel.
//
//  * sort / argsort records (layouts.rs:1158-1275 `_sort_ascending` and the claimed indices of `shuffles`, :1624-1760: the one step of the
//    layout engine whose cell ORDER depends on the values): segments of n cells sorted by (signed value, position) -- a total order, so a
//    bitonic network gives the cells of any other correct sort -- see wit_sort_lds_kernel: SORT_TILE keys per workgroup in LDS, whole
//    segments side by side when they are short; a longer segment goes through the plan's key scratch, one launch per stride at or above
//    the tile and one LDS launch for the strides below it.  A source beyond 62 bits is reported as the range failures below are ("sort
//    key beyond 62 bits") and its segment writes none of its cells.
//
//  * recip / sqrt records (the claims of layouts.rs:300-385 `recip` and :408-459 `sqrt`, which the reference computes in f64 and enforces
//    with `optimum_convex_function`, :114-143): element-wise, one lane per destination cell, exact 64-bit integers.  recip: the smallest
//    integer minimiser of |y * x - S| in closed form -- x > 0: (2S + x - 1) / (2x), x < 0: -((2S + |x|) / (2|x|)), one unsigned 64-bit
//    division per lane (a software sequence on this hardware, small beside the two Montgomery conversions of the lane); x = 0 takes the
//    circuit's zero_inverse constant.  This is the value the gates accept: where x > 0 divides 2S but not S the f64 formula rounds the
//    tie up and the gates refuse it.  sqrt: T = x * scale, the floor root from a double estimate corrected by integer comparison, then
//    r + (T - r^2 > r).  An operand beyond 62 bits, or T >= 2^62, is reported as the range failures below are ("reciprocal operand beyond
//    62 bits", "square-root operand outside the exact range") and writes nothing.
//
//  * arg-extremum records (the index `argmax` / `argmin` claim before the sort that checks it, layouts.rs:5225-5293): count segments of n
//    source cells, one destination cell each -- the smallest position of the greatest (least) signed value.  See wit_argext_wave_kernel: up
//    to 64 sources a segment, whole segments side by side in a wave and cross-lane steps only; up to ARGEXT_CHUNK, a workgroup per segment;
//    above, a workgroup per chunk into the plan's key scratch and a second launch over the slots.  A source beyond 62 bits is reported as
//    the range failures below are ("arg-extremum key beyond 62 bits") and its segment's cell is not written.
//
//  * scatter / complement / one-hot records (the three claims of the indexed family that depend on the data -- layouts.rs:2313-2379
//    `scatter_elements`, :2213-2286 `get_missing_set_elements`, :1398-1442 `one_hot`): the scattered tensor by a last-writer-wins scatter --
//    an atomicMax of the element number per target, so the result does not depend on scheduling --, the positions no index names by mark, scan
//    and compact, the one-hot vector element-wise.  See wit_scatter_lds_kernel and wit_compl_lds_kernel: up to SCATTER_TILE destinations one
//    workgroup in LDS, above it launches through the plan's scratch.  A scatter index outside its dimension is reported as the range failures
//    below are ("scatter index outside the tensor") and its record writes none of its cells; a one-hot index outside the classes likewise
//    ("one-hot index outside the classes"); a complement never fails.
//
// A value that does not fit its decomposition (|x| >= base^legs: the layout's "value exceeds the decomposition range") writes nothing
// wrong silently, and neither does a lookup input outside its table (layouts.rs:5143-5222 `nonlinearity`; the layout's "lookup input
// outside the table range"), and neither does a dividend of `div` beyond the range in which the integer quotient is the reference's f64
// one (|s| >= 2^52: "rebase dividend outside the exact-division range"): the lane counts itself in status[0] and keeps the SMALLEST
// (record, element) in status[1] -- vector atomics in plain C++, as the mock prover's kernels in vecops.hip -- and the host call
// returns EZKL_ERR_INVALID naming the op.  Nothing traps.
// The only device memory written is the destination columns, the plan's own scratch (inputs, outputs, sort keys, arg-extremum slots, scatter winners or complement flags, the three words of the lookup statistics) and the status words; the plan's
// index pool, parameters, constants and lookup-table values are read-only after upload.
#include "common.hpp"
#include "witness_plan.hpp"
#include <atomic>

namespace ezkl {
namespace {
using namespace wplan;

struct WitCols {
    fe_t* p[MAX_ADVICE];
};
// status words on the device: [0] failing lanes, [1] ~(record << 32 | element) of the first one (atomicMax over the complement: zero = none),
// [2] cells written
EZ_D fe_t* wit_cell(const WitCols& cols, uint32_t k, uint32_t idx) { return cols.p[idx >> k] + (idx & ((1u << k) - 1)); }

// integer_rep_to_felt (/root/reference/src/fieldutils.rs:9-17) as msm_expand_integer_rep_kernel does it for EZKL_COLUMN_INT64: x >= 0 -> x,
// x < 0 -> r - |x|, then the Montgomery form
EZ_D fe_t wit_from_i64(int64_t x) {
    const bool neg = x < 0;
    const uint64_t m = neg ? ~(uint64_t)x + 1 : (uint64_t)x;
    fe_t v = Fr::zero();
    v.v[0] = (uint32_t)m; v.v[1] = (uint32_t)(m >> 32);
    if (neg) {
        uint32_t br = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) v.v[i] = subb32(FrP::MOD[i], v.v[i], br);
    }
    return Fr::to_mont(v);
}
EZ_HD constexpr uint32_t wit_half(int i) { return (FrP::MOD[i] >> 1) | (i < 7 ? (FrP::MOD[i + 1] << 31) : 0u); }   // limb i of (r - 1) / 2
// the signed value of a Montgomery word as the layout reads it (`v if v < r // 2 else v - r`): sign and magnitude.  fits: |x| < 2^62.
EZ_D void wit_signed(const fe_t& mont, bool& neg, uint64_t& mag, bool& fits) {
    const fe_t c = Fr::from_mont(mont);
    uint32_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) (void)subb32(c.v[i], wit_half(i), br);
    neg = br == 0;                                        // c >= (r - 1) / 2
    fe_t m = c;
    if (neg) {
        br = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) m.v[i] = subb32(FrP::MOD[i], c.v[i], br);
    }
    uint32_t hi = m.v[1] >> 30;
#pragma unroll
    for (int i = 2; i < 8; i++) hi |= m.v[i];
    fits = hi == 0;
    mag = (uint64_t)m.v[0] | ((uint64_t)m.v[1] << 32);
}
EZ_D void wit_report(bool fail, uint32_t rec, uint32_t elem, unsigned long long* status) {
    const unsigned long long m = __ballot(fail);
    if (!m) return;
    if ((threadIdx.x & 63) == (uint32_t)__ffsll(m) - 1) atomicAdd(&status[0], (unsigned long long)__popcll(m));
    if (fail) atomicMax(&status[1], ~(((unsigned long long)rec << 32) | elem));
}
EZ_D void wit_count(uint32_t wrote, unsigned long long* status) {          // one atomic per wave
#pragma unroll
    for (int off = 32; off; off >>= 1) wrote += __shfl_down(wrote, off);
    if ((threadIdx.x & 63) == 0 && wrote) atomicAdd(&status[2], (unsigned long long)wrote);
}

template <uint32_t KIND>
__global__ __launch_bounds__(256) void wit_elem_kernel(WitCols cols, uint32_t k, const uint32_t* __restrict__ dst, const uint32_t* __restrict__ a,
                                                       const uint32_t* __restrict__ b, uint32_t count, uint32_t p0, uint32_t p1, uint32_t p2,
                                                       const int64_t* __restrict__ ints, const fe_t* __restrict__ consts, uint32_t rec,
                                                       unsigned long long* status) {
    // TABLE / TBLIDX: the launcher has resolved the table directory -- ints = the table's values, p0 = lo (int32), p1 = n, p2 = col_size
    // GATHER: b = the table's cell list (pool + p0), p1 = its length
    // RECIP: p0 | p1 << 32 = S, p2 = the index in consts of the value a zero input takes; ISQRT: p0 = the input scale
    // ONEHOT: b = the position each element stands for, p0 = the number of classes
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < count;
    bool fail = false;
    if (live) {
        const uint32_t ia = a[i];
        fe_t v;
        if (KIND == COPY) v = ld_fe(wit_cell(cols, k, ia));
        else if (KIND == CONST) v = ld_fe(consts + ia);
        else if (KIND == INPUT || KIND == PARAM) v = wit_from_i64(ints[ia]);
        else if (KIND == ADD) v = Fr::add(ld_fe(wit_cell(cols, k, ia)), ld_fe(wit_cell(cols, k, b[i])));
        else if (KIND == SUB) v = Fr::sub(ld_fe(wit_cell(cols, k, ia)), ld_fe(wit_cell(cols, k, b[i])));
        else if (KIND == MUL) v = Fr::mul(ld_fe(wit_cell(cols, k, ia)), ld_fe(wit_cell(cols, k, b[i])));
        else if (KIND == INVZ) v = Fr::inv(ld_fe(wit_cell(cols, k, ia)));                    // a^(r-2): inv(0) = 0
        else {
            bool neg, fits;
            uint64_t mag;
            wit_signed(ld_fe(wit_cell(cols, k, ia)), neg, mag, fits);
            if (KIND == HINT) {
                uint64_t bound = 1;
                for (uint32_t t = 0; t < p1; t++) bound *= p0;                                // < 2^62: checked on upload
                fail = !fits || mag >= bound;
                const uint32_t e = b[i];
                if (e == NONE) v = mag == 0 ? Fr::zero() : neg ? Fr::neg(Fr::one()) : Fr::one();
                else {
                    uint64_t d = 1;
                    for (uint32_t t = 0; t < e; t++) d *= p0;
                    v = Fr::from_u64((mag / d) % p0);
                }
            } else if (KIND == DIVC) {                                                        // sgn(s) * ((|s| + d / 2) / d), d = p0 >= 1: checked on upload
                fail = !fits || (mag >> 52) != 0;
                if (!fail) {
                    const uint64_t q = (mag + p0 / 2) / p0;                                   // < 2^52 + 2^31
                    v = wit_from_i64(neg ? -(int64_t)q : (int64_t)q);
                }
            } else if (KIND == GATHER) {                                                      // the cell b[s], 0 <= s < p1: tested before b[s] is read
                fail = !fits || neg || mag >= p1;
                if (!fail) v = ld_fe(wit_cell(cols, k, b[mag]));
            } else if (KIND == CLAMP) {                                                       // min(max(s, lo), hi); beyond 62 bits: by the sign
                const int64_t lo = (int32_t)p0, hi = (int32_t)p1;
                int64_t s = neg ? lo : hi;
                if (fits) {
                    s = neg ? -(int64_t)mag : (int64_t)mag;
                    s = s < lo ? lo : s > hi ? hi : s;
                }
                v = wit_from_i64(s);
            } else if (KIND == RECIP) {                                                       // the smallest integer minimiser of |y * x - S|, S = p0 | p1 << 32
                fail = !fits;
                if (!fail) {
                    if (mag == 0) v = ld_fe(consts + p2);                                     // zero_inverse: p2 = its constant index, checked on upload
                    else {                                                                    // S < 2^62 (upload), mag < 2^62 (fits): 2S + mag < 2^64, 2 mag < 2^63
                        const uint64_t S = (uint64_t)p0 | ((uint64_t)p1 << 32);
                        const uint64_t q = (2 * S + mag - (neg ? 0 : 1)) / (2 * mag);          // x > 0: ceil((2S - x) / (2x)); x < 0: floor((2S + |x|) / (2|x|))
                        v = wit_from_i64(neg ? -(int64_t)q : (int64_t)q);                     // q <= S + 1 / 2 < 2^62
                    }
                }
            } else if (KIND == ISQRT) {                                                       // the integer nearest to sqrt(T), T = x * p0; T <= 0: zero
                const uint64_t T = mag * p0;                                                  // the low word; the high one decides with it whether T fits
                fail = !fits || (!neg && (__umul64hi(mag, (uint64_t)p0) != 0 || (T >> 62) != 0));
                if (!fail) {
                    uint64_t r = 0;
                    if (!neg && T) {
                        r = (uint64_t)sqrt((double)T);                                        // within one of the floor root: T < 2^62, the estimate is off by < 2^-20
                        if (r > 0x7fffffffull) r = 0x7fffffffull;                             // floor(sqrt(2^62 - 1)) = 2^31 - 1: r * r and (r + 1)^2 below fit 64 bits
#pragma unroll
                        for (int t = 0; t < 2; t++) {                                         // corrected by integer comparison, both ways
                            if (r * r > T) r--;
                            else if ((r + 1) * (r + 1) <= T) r++;
                        }
                        r += (T - r * r > r) ? 1 : 0;                                         // T - r^2 > r  <=>  T > (r + 1/2)^2: the nearer integer is r + 1
                    }
                    v = Fr::from_u64(r);
                }
            } else if (KIND == ONEHOT) {                                                      // 1 at the position the index names, 0 <= s < p0 classes
                fail = !fits || neg || mag >= p0;
                if (!fail) v = mag == b[i] ? Fr::one() : Fr::zero();
            } else if (KIND == RCIDX) {                                                       // |x - lo| // col_size
                fail = !fits;                                                                 // |x| >= 2^62: as run_plan_host refuses it
                const int64_t s = neg ? -(int64_t)mag : (int64_t)mag, diff = s - (int64_t)(int32_t)p0;
                v = Fr::from_u64((uint64_t)(diff < 0 ? -diff : diff) / p1);
            } else {                                                                          // TABLE: values[s - lo]; TBLIDX: (s - lo) // col_size
                fail = !fits;                                                                 // |s| >= 2^62: outside every table
                if (fits) {
                    const int64_t s = neg ? -(int64_t)mag : (int64_t)mag, diff = s - (int64_t)(int32_t)p0;
                    fail = diff < 0 || diff >= (int64_t)p1;                                   // outside [lo, lo + n - 1]: nothing is read
                    if (!fail) v = KIND == TABLE ? wit_from_i64(ints[diff]) : Fr::from_u64((uint64_t)diff / p2);
                }
            }
        }
        if (!fail) st_fe(wit_cell(cols, k, dst[i]), v);
    }
    wit_report(fail, rec, i, status);
    wit_count(live && !fail ? 1u : 0u, status);
}

// DOT_LANES consecutive lanes share one dot product; step s of dot d: dst[s * n_dots + d], products (a, b)[(s * w + j) * n_dots + d], j < w.
// The rows of a dot are cut into DOT_LANES contiguous chunks.  Pass 1: every lane sums the products of its chunk.  A scan over the
// group's lanes (wave shuffles, no LDS) gives each lane the running sum at the start of its chunk.  Pass 2: the lane walks its chunk
// again and writes the running sum of every row.  Field addition is exact, so the sums are those of the row-by-row walk bit for bit.
constexpr uint32_t DOT_LANES = 16;
EZ_D fe_t wit_shfl_up(const fe_t& v, uint32_t delta) {
    fe_t r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = __shfl_up(v.v[i], delta, DOT_LANES);
    return r;
}
EZ_D fe_t wit_dot_row(const WitCols& cols, uint32_t k, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t n_dots, uint32_t w, uint32_t s,
                      uint32_t d, fe_t acc) {
    for (uint32_t j = 0; j < w; j++) {
        const size_t at = ((size_t)s * w + j) * n_dots + d;
        const uint32_t ia = a[at];
        if (ia != NONE) acc = Fr::add(acc, Fr::mul(ld_fe(wit_cell(cols, k, ia)), ld_fe(wit_cell(cols, k, b[at]))));
    }
    return acc;
}
__global__ __launch_bounds__(64) void wit_dot_kernel(WitCols cols, uint32_t k, const uint32_t* __restrict__ dst, const uint32_t* __restrict__ a,
                                                     const uint32_t* __restrict__ b, uint32_t n_dots, uint32_t w, uint32_t n_steps,
                                                     unsigned long long* status) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t g = (uint32_t)(t % DOT_LANES), chunk = (n_steps + DOT_LANES - 1) / DOT_LANES;
    const bool live = t / DOT_LANES < n_dots;                    // the same for every lane of a group
    const uint32_t d = live ? (uint32_t)(t / DOT_LANES) : 0;
    const uint32_t s0 = g * chunk < n_steps ? g * chunk : n_steps, s1 = s0 + chunk < n_steps ? s0 + chunk : n_steps;
    fe_t sum = Fr::zero();
    if (live)
        for (uint32_t s = s0; s < s1; s++)
            if (dst[(size_t)s * n_dots + d] != NONE) sum = wit_dot_row(cols, k, a, b, n_dots, w, s, d, sum);
    for (uint32_t off = 1; off < DOT_LANES; off <<= 1) {           // inclusive scan of the chunk sums over the group
        const fe_t o = wit_shfl_up(sum, off);
        if (g >= off) sum = Fr::add(sum, o);
    }
    fe_t acc = wit_shfl_up(sum, 1);                               // exclusive: the running sum before this lane's first row
    if (g == 0) acc = Fr::zero();
    uint32_t wrote = 0;
    if (live)
        for (uint32_t s = s0; s < s1; s++) {
            const uint32_t cell = dst[(size_t)s * n_dots + d];
            if (cell == NONE) continue;
            acc = wit_dot_row(cols, k, a, b, n_dots, w, s, d, acc);
            st_fe(wit_cell(cols, k, cell), acc);
            wrote++;
        }
    wit_count(wrote, status);
}

// A DOT record of one step (n_steps == 1) with many products: the claimed product of an einsum, dot d = sum_j a[j * n_dots + d] * b[...], j < w,
// written to dst[d].  wit_dot_kernel would cut the ONE step into 16 chunks and leave 15 lanes of 16 idle; here every lane multiplies.  A wave
// holds 64 / G dots, G lanes to a dot (G a power of two the host chooses, dot_wide_lanes): lane l works on dot l % (64 / G) and takes the
// products j = l / (64 / G), + G, + 2G, ... -- so the 64 / G lanes with the same j read consecutive index words (the arrays are j-major, dense
// along d), for G = 1 a whole wave does.  Two running sums per lane keep two Montgomery products in flight.  The partial sums of a dot sit
// 64 / G lanes apart and are added by a butterfly of wave shuffles; the lane with j = 0 writes.  Field addition is exact and Fr::add answers
// the canonical word, so the cell is wit_dot_kernel's bit for bit whatever the order of the additions.
EZ_D fe_t wit_shfl_xor(const fe_t& v, uint32_t mask) {
    fe_t r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = __shfl_xor(v.v[i], (int)mask, 64);
    return r;
}
EZ_D fe_t wit_product(const WitCols& cols, uint32_t k, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, size_t at, fe_t acc) {
    const uint32_t ia = a[at];
    if (ia != NONE) acc = Fr::add(acc, Fr::mul(ld_fe(wit_cell(cols, k, ia)), ld_fe(wit_cell(cols, k, b[at]))));
    return acc;
}
__global__ __launch_bounds__(64) void wit_dot_wide_kernel(WitCols cols, uint32_t k, const uint32_t* __restrict__ dst, const uint32_t* __restrict__ a,
                                                          const uint32_t* __restrict__ b, uint32_t n_dots, uint32_t w, uint32_t lanes,
                                                          unsigned long long* status) {
    const uint32_t per_wave = 64 / lanes, l = threadIdx.x & 63;
    const size_t d = (size_t)blockIdx.x * per_wave + l % per_wave;
    const uint32_t g = l / per_wave;
    const uint32_t cell = d < n_dots ? dst[d] : NONE;            // the same for every lane of a dot; no destination: no products either
    fe_t s0 = Fr::zero(), s1 = Fr::zero();
    if (cell != NONE) {
        uint32_t j = g;
        for (; j + lanes < w; j += 2 * lanes) {
            s0 = wit_product(cols, k, a, b, (size_t)j * n_dots + d, s0);
            s1 = wit_product(cols, k, a, b, (size_t)(j + lanes) * n_dots + d, s1);
        }
        if (j < w) s0 = wit_product(cols, k, a, b, (size_t)j * n_dots + d, s0);
    }
    fe_t sum = Fr::add(s0, s1);
    for (uint32_t off = per_wave; off < 64; off <<= 1) sum = Fr::add(sum, wit_shfl_xor(sum, off));     // every lane of the wave takes part
    const bool write = cell != NONE && g == 0;
    if (write) st_fe(wit_cell(cols, k, cell), sum);
    wit_count(write ? 1u : 0u, status);
}

// The running sum (SUMACC) or product (PRODACC) of w cells per row: wit_dot_kernel with one operand per entry and the fold as the monoid.
// DOT_LANES consecutive lanes share one scan; step s of scan d: dst[s * n_scans + d], operands a[(s * w + j) * n_scans + d], j < w
// (0xffffffff: none).  Pass 1: a lane folds its chunk of steps from the identity.  The shuffle scan over the group's lanes gives each
// lane the running value at the start of its chunk.  Pass 2: the lane walks its chunk again and writes every row.  Field addition and
// the Montgomery product are exact, associative and commutative: the bits are those of the row-by-row walk.
template <uint32_t KIND>
EZ_D fe_t wit_fold(const fe_t& x, const fe_t& y) { return KIND == SUMACC ? Fr::add(x, y) : Fr::mul(x, y); }
template <uint32_t KIND>
EZ_D fe_t wit_acc_row(const WitCols& cols, uint32_t k, const uint32_t* __restrict__ a, uint32_t n_scans, uint32_t w, uint32_t s, uint32_t d, fe_t acc) {
    for (uint32_t j = 0; j < w; j++) {
        const uint32_t ia = a[((size_t)s * w + j) * n_scans + d];
        if (ia != NONE) acc = wit_fold<KIND>(acc, ld_fe(wit_cell(cols, k, ia)));
    }
    return acc;
}
template <uint32_t KIND>
__global__ __launch_bounds__(64) void wit_acc_kernel(WitCols cols, uint32_t k, const uint32_t* __restrict__ dst, const uint32_t* __restrict__ a, uint32_t n_scans,
                                                     uint32_t w, uint32_t n_steps, unsigned long long* status) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t g = (uint32_t)(t % DOT_LANES), chunk = (n_steps + DOT_LANES - 1) / DOT_LANES;
    const bool live = t / DOT_LANES < n_scans;                   // the same for every lane of a group
    const uint32_t d = live ? (uint32_t)(t / DOT_LANES) : 0;
    const uint32_t s0 = g * chunk < n_steps ? g * chunk : n_steps, s1 = s0 + chunk < n_steps ? s0 + chunk : n_steps;
    const fe_t id = KIND == SUMACC ? Fr::zero() : Fr::one();
    fe_t run = id;
    if (live)
        for (uint32_t s = s0; s < s1; s++)
            if (dst[(size_t)s * n_scans + d] != NONE) run = wit_acc_row<KIND>(cols, k, a, n_scans, w, s, d, run);
    for (uint32_t off = 1; off < DOT_LANES; off <<= 1) {           // inclusive scan of the chunk folds over the group
        const fe_t o = wit_shfl_up(run, off);
        if (g >= off) run = wit_fold<KIND>(run, o);
    }
    fe_t acc = wit_shfl_up(run, 1);                               // exclusive: the running value before this lane's first row
    if (g == 0) acc = id;
    uint32_t wrote = 0;
    if (live)
        for (uint32_t s = s0; s < s1; s++) {
            const uint32_t cell = dst[(size_t)s * n_scans + d];
            if (cell == NONE) continue;
            acc = wit_acc_row<KIND>(cols, k, a, n_scans, w, s, d, acc);
            st_fe(wit_cell(cols, k, cell), acc);
            wrote++;
        }
    wit_count(wrote, status);
}

// sign and magnitude (< 2^127, two words) -> integer_rep_to_felt -> Montgomery form
EZ_D fe_t wit_from_mag128(bool neg, uint64_t lo, uint64_t hi) {
    fe_t v = Fr::zero();
    v.v[0] = (uint32_t)lo; v.v[1] = (uint32_t)(lo >> 32); v.v[2] = (uint32_t)hi; v.v[3] = (uint32_t)(hi >> 32);
    if (neg && (lo | hi)) {
        uint32_t br = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) v.v[i] = subb32(FrP::MOD[i], v.v[i], br);
    }
    return Fr::to_mont(v);
}

// dst[i * n + j] = sum_t in[a[i * kd + t]] * in[b[t * n + j]] over the integers: MM_TILE x MM_TILE outputs per block, one per lane.  Per
// k-step of MM_TILE every lane loads ONE operand of A and ONE of B through the index arrays into LDS -- checked there, once, for
// |v| < 2^31, so the tiles hold int32 and a product is an exact int64 below 2^62 in magnitude -- and adds MM_TILE products into a
// two-word accumulator (kd * 2^62 < 2^127).  Positions past m, n or kd load zeros.  A block that met a bad operand writes nothing:
// every one of its outputs would read it or a neighbour's; the lane that loaded it reports (record, element) with element = the
// operand's place in a, or m * kd + its place in b.
constexpr uint32_t MM_TILE = 16;
__global__ __launch_bounds__(MM_TILE * MM_TILE) void wit_matmul_kernel(WitCols cols, uint32_t k, const uint32_t* __restrict__ dst, const uint32_t* __restrict__ a,
                                                                     const uint32_t* __restrict__ b, uint32_t m, uint32_t kd, uint32_t n,
                                                                     const int64_t* __restrict__ in, uint32_t rec, unsigned long long* status) {
    __shared__ int32_t As[MM_TILE][MM_TILE + 1], Bs[MM_TILE][MM_TILE + 1];
    const uint32_t tiles_n = (n + MM_TILE - 1) / MM_TILE;
    const uint32_t tx = threadIdx.x % MM_TILE, ty = threadIdx.x / MM_TILE;
    const uint32_t i = (blockIdx.x / tiles_n) * MM_TILE + ty, j = (blockIdx.x % tiles_n) * MM_TILE + tx;
    uint64_t lo = 0;
    int64_t hi = 0;
    bool bad = false;
    uint32_t bad_elem = 0xFFFFFFFFu;
    for (uint32_t t0 = 0; t0 < kd; t0 += MM_TILE) {
        int64_t va = 0, vb = 0;
        if (i < m && t0 + tx < kd) {                         // A[i][t0 + tx]
            const uint32_t e = i * kd + t0 + tx;
            va = in[a[e]];
            if (va >= ((int64_t)1 << 31) || va <= -((int64_t)1 << 31)) { bad = true; bad_elem = bad_elem < e ? bad_elem : e; va = 0; }
        }
        if (t0 + ty < kd && j < n) {                         // B[t0 + ty][j]
            const uint32_t e = (t0 + ty) * n + j;
            vb = in[b[e]];
            if (vb >= ((int64_t)1 << 31) || vb <= -((int64_t)1 << 31)) { bad = true; bad_elem = bad_elem < m * kd + e ? bad_elem : m * kd + e; vb = 0; }
        }
        As[ty][tx] = (int32_t)va;
        Bs[ty][tx] = (int32_t)vb;
        __syncthreads();
#pragma unroll
        for (uint32_t t = 0; t < MM_TILE; t++) {
            const int64_t p = (int64_t)As[ty][t] * (int64_t)Bs[t][tx];
            lo += (uint64_t)p;
            hi += (p >> 63) + (lo < (uint64_t)p ? 1 : 0);
        }
        __syncthreads();
    }
    const bool block_bad = __syncthreads_or(bad ? 1 : 0) != 0;
    const bool live = i < m && j < n && !block_bad;
    if (live) {
        const bool neg = hi < 0;
        uint64_t mlo = lo, mhi = (uint64_t)hi;
        if (neg) {
            mlo = ~lo + 1;
            mhi = ~(uint64_t)hi + (mlo == 0 ? 1 : 0);
        }
        st_fe(wit_cell(cols, k, dst[i * n + j]), wit_from_mag128(neg, mlo, mhi));
    }
    wit_report(bad, rec, bad_elem, status);
    wit_count(live ? 1u : 0u, status);
}

// RLC_LANES consecutive lanes share one scan out[t] = c * (out[t-1] + v[t]) (= out[t-1] * c + c * v[t]: field arithmetic is exact), out[-1] = 0;
// step t of scan d reads cell a[t * n_scans + d] and writes cell dst[t * n_scans + d].  The chunked scan of wit_dot_kernel with an
// affine map in the combine step.  Pass 1: a lane folds its chunk from zero (S) and builds P = c^len as it goes: the chunk maps a
// carried-in x to P * x + S.  The shuffle scan over the group composes the maps -- (P1, S1) then (P2, S2) is (P1 * P2, S1 * P2 + S2) --
// so S of the lane before is the running value at the start of a lane's chunk.  Pass 2: the lane walks its chunk again from the
// carried-in value and writes every row: the bits of the row-by-row walk.
constexpr uint32_t RLC_LANES = DOT_LANES;
__global__ __launch_bounds__(64) void wit_rlc_kernel(WitCols cols, uint32_t k, const uint32_t* __restrict__ dst, const uint32_t* __restrict__ a, uint32_t n_scans,
                                                     uint32_t n_steps, fe_t c, unsigned long long* status) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t g = (uint32_t)(t % RLC_LANES), chunk = (n_steps + RLC_LANES - 1) / RLC_LANES;
    const bool live = t / RLC_LANES < n_scans;                   // the same for every lane of a group
    const uint32_t d = live ? (uint32_t)(t / RLC_LANES) : 0;
    const uint32_t s0 = g * chunk < n_steps ? g * chunk : n_steps, s1 = s0 + chunk < n_steps ? s0 + chunk : n_steps;
    fe_t S = Fr::zero(), P = Fr::one();
    if (live)
        for (uint32_t s = s0; s < s1; s++) {
            S = Fr::mul(c, Fr::add(S, ld_fe(wit_cell(cols, k, a[(size_t)s * n_scans + d]))));
            P = Fr::mul(P, c);
        }
    for (uint32_t off = 1; off < RLC_LANES; off <<= 1) {           // inclusive scan of the chunk maps over the group: the earlier map first
        const fe_t Po = wit_shfl_up(P, off), So = wit_shfl_up(S, off);
        if (g >= off) {
            S = Fr::add(Fr::mul(So, P), S);
            P = Fr::mul(Po, P);
        }
    }
    fe_t acc = wit_shfl_up(S, 1);                                 // exclusive: the running value before this lane's first row
    if (g == 0) acc = Fr::zero();
    uint32_t wrote = 0;
    if (live)
        for (uint32_t s = s0; s < s1; s++) {
            acc = Fr::mul(c, Fr::add(acc, ld_fe(wit_cell(cols, k, a[(size_t)s * n_scans + d]))));
            st_fe(wit_cell(cols, k, dst[(size_t)s * n_scans + d]), acc);
            wrote++;
        }
    wit_count(wrote, status);
}

__global__ __launch_bounds__(64) void wit_gather_kernel(WitCols cols, uint32_t k, const uint32_t* __restrict__ cells, uint32_t n, fe_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) st_fe(out + i, ld_fe(wit_cell(cols, k, cells[i])));
}

// ezkl_hip_witness_lookup_stats_dev: the least and the greatest signed input of every static lookup of a replayed plan, folded with 0 --
// what BaseRegion.nonlinearity keeps on the host as min_lookup_inputs / max_lookup_inputs (the reference's src/circuit/ops/region.rs:548-559).
// recs: (pool offset of the source cells, count) of every TABLE record; one lane per element, the grid striding over each record in
// turn; the extrema are reduced across the wave in registers and leave it through one signed 64-bit atomicMin and one atomicMax on
// out[0] / out[1], which the host call has set to 0; a source beyond 62 bits is counted in out[2] instead and the call refuses the result.
// Every index read here was checked on upload: a TABLE record's sources are cells below n_advice * 2^k.
struct StatRec {
    uint32_t a, count;
};
constexpr uint32_t STATS_THREADS = 256, STATS_MAX_BLOCKS = 256;             // at most a workgroup per CU: past 2^16 elements the lanes stride
__global__ __launch_bounds__(STATS_THREADS) void wit_lookup_stats_kernel(WitCols cols, uint32_t k, const uint32_t* __restrict__ pool, const StatRec* __restrict__ recs,
                                                                         uint32_t n_recs, long long* __restrict__ out) {
    const uint64_t first = (uint64_t)blockIdx.x * STATS_THREADS + threadIdx.x, stride = (uint64_t)gridDim.x * STATS_THREADS;
    int64_t lo = 0, hi = 0;
    uint32_t bad = 0;
    for (uint32_t r = 0; r < n_recs; r++) {
        const StatRec rec = recs[r];
        const uint32_t* __restrict__ a = pool + rec.a;
        for (uint64_t i = first; i < rec.count; i += stride) {
            bool neg, fits;
            uint64_t mag;
            wit_signed(ld_fe(wit_cell(cols, k, a[i])), neg, mag, fits);
            const int64_t s = neg ? -(int64_t)mag : (int64_t)mag;          // |s| < 2^62 where it fits
            bad += fits ? 0u : 1u;
            lo = fits && s < lo ? s : lo;
            hi = fits && s > hi ? s : hi;
        }
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const uint32_t l0 = (uint32_t)__shfl_xor((int)(uint32_t)lo, off), l1 = (uint32_t)__shfl_xor((int)(uint32_t)((uint64_t)lo >> 32), off);
        const uint32_t h0 = (uint32_t)__shfl_xor((int)(uint32_t)hi, off), h1 = (uint32_t)__shfl_xor((int)(uint32_t)((uint64_t)hi >> 32), off);
        const int64_t ylo = (int64_t)((uint64_t)l0 | ((uint64_t)l1 << 32)), yhi = (int64_t)((uint64_t)h0 | ((uint64_t)h1 << 32));
        lo = ylo < lo ? ylo : lo;
        hi = yhi > hi ? yhi : hi;
        bad += (uint32_t)__shfl_xor((int)bad, off);
    }
    if ((threadIdx.x & 63) == 0) {                                          // one atomic of each per wave, none where the wave changes nothing
        if (lo < 0) atomicMin(&out[0], (long long)lo);
        if (hi > 0) atomicMax(&out[1], (long long)hi);
        if (bad) atomicAdd(reinterpret_cast<unsigned long long*>(&out[2]), (unsigned long long)bad);
    }
}

// ezkl_hip_witness_tile_dev: rows [t * U, (t + 1) * U) of dst[pair] get rows [0, U) of src[pair].  One lane per destination cell, a
// 32-byte copy each; consecutive lanes take consecutive rows, so both sides coalesce.  Grid: x over the T * U rows, y over the pairs.
// A self-pair (dst == src) skips t = 0: it reads rows [0, U) and writes rows [U, T * U) of its column, disjoint by construction, and
// the host has refused a source that is another pair's destination -- no lane reads a cell that a lane of this launch writes.
struct WitTile {
    fe_t* dst[MAX_ADVICE];
    const fe_t* src[MAX_ADVICE];
};
__global__ __launch_bounds__(256) void wit_tile_kernel(WitTile t, uint32_t unit_rows, uint32_t rows) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;       // rows = T * U <= 2^28
    fe_t* dst = t.dst[blockIdx.y];
    const fe_t* src = t.src[blockIdx.y];
    if (i >= rows || (dst == src && i < unit_rows)) return;
    st_fe(dst + i, ld_fe(src + i % unit_rows));
}

// SORT / ARGSORT.  A key is (signed value, tie) with tie = the element's position in its segment (mode 0) or n - 1 - position (mode 1), compared
// lexicographically; a segment of n keys is padded with (INT64_MAX, 0xffffffff) to P = the next power of two.  A source beyond 62 bits
// enters as (INT64_MAX, 0xfffffffe): above every key that fits, below the pads.  So after the sort the key at place n - 1 of a segment is
// the segment's flag -- value INT64_MAX: some source did not fit, none of the segment's cells is written -- rewritten by every run, in
// LDS or in the scratch, never status[0], which an earlier record may have set.  The network: stage `size` = 2, 4 .. P, strides size / 2
// .. 1; the pair (i, i | stride) is put in ascending order when bit `size` of i's place in its segment is clear, in descending order
// otherwise (the last stage, size = P, is ascending throughout).  Every loop bound is a function of P and SORT_TILE.
struct alignas(16) SortKey {
    int64_t v;
    uint32_t tie, pad;
};
constexpr int64_t SORT_PAD = INT64_MAX;
constexpr uint32_t SORT_THREADS = 256, SORT_TIE_PAD = 0xFFFFFFFFu, SORT_TIE_BAD = 0xFFFFFFFEu;
static_assert(SORT_TILE % (2 * SORT_THREADS) == 0 && (SORT_TILE & (SORT_TILE - 1)) == 0, "a tile is a power of two of whole rounds of pairs");

// the key of source element e = seg * n + i of record `rec` (live: the element exists), reported when it does not fit
EZ_D void wit_sort_load(const WitCols& cols, uint32_t k, const uint32_t* __restrict__ a, bool live, size_t e, uint32_t i, uint32_t n, uint32_t mode, uint32_t rec,
                        unsigned long long* status, int64_t& v, uint32_t& tie) {
    v = SORT_PAD; tie = SORT_TIE_PAD;
    bool fail = false;
    if (live) {
        bool neg, fits;
        uint64_t mag;
        wit_signed(ld_fe(wit_cell(cols, k, a[e])), neg, mag, fits);
        fail = !fits;
        v = fail ? SORT_PAD : neg ? -(int64_t)mag : (int64_t)mag;
        tie = fail ? SORT_TIE_BAD : mode ? n - 1 - i : i;
    }
    wit_report(fail, rec, (uint32_t)e, status);
}
EZ_D bool wit_sort_above(int64_t xv, uint32_t xt, int64_t yv, uint32_t yt) { return xv > yv || (xv == yv && xt > yt); }
// strides stride0, stride0 / 2 .. 1 of stage `size` on the SORT_TILE keys in LDS; `base`: the place in its segment of slot 0, P - 1: mask
EZ_D void wit_sort_lds_strides(int64_t* key, uint32_t* tie, uint32_t base, uint32_t mask, uint32_t size, uint32_t stride0) {
    for (uint32_t stride = stride0; stride; stride >>= 1) {
        __syncthreads();
#pragma unroll
        for (uint32_t q = 0; q < SORT_TILE / (2 * SORT_THREADS); q++) {
            const uint32_t t = threadIdx.x + q * SORT_THREADS;
            const uint32_t i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), j = i | stride;       // j < SORT_TILE: t < SORT_TILE / 2
            const bool asc = (((base + i) & mask) & size) == 0;
            const int64_t xv = key[i], yv = key[j];
            const uint32_t xt = tie[i], yt = tie[j];
            if (wit_sort_above(xv, xt, yv, yt) == asc) {
                key[i] = yv; key[j] = xv;
                tie[i] = yt; tie[j] = xt;
            }
        }
    }
    __syncthreads();
}
// what destination element (seg, i) gets from the key at its place: the value, or the position the tie stands for
template <uint32_t KIND>
EZ_D fe_t wit_sort_out(int64_t v, uint32_t tie, uint32_t n, uint32_t mode) {
    return KIND == SORT ? wit_from_i64(v) : Fr::from_u64(mode ? n - 1 - tie : tie);
}

// P <= SORT_TILE: one workgroup sorts SORT_TILE / P whole segments, slot j of the tile = element j % P of segment blockIdx.x * (SORT_TILE / P)
// + j / P.  Load (wit_signed), the network in LDS up to size P, store.
template <uint32_t KIND>
__global__ __launch_bounds__(SORT_THREADS) void wit_sort_lds_kernel(WitCols cols, uint32_t k, const uint32_t* __restrict__ dst, const uint32_t* __restrict__ a,
                                                                    uint32_t n_segs, uint32_t n, uint32_t P, uint32_t mode, uint32_t rec, unsigned long long* status) {
    __shared__ int64_t key[SORT_TILE];
    __shared__ uint32_t tie[SORT_TILE];
    const uint32_t per = SORT_TILE / P, seg0 = blockIdx.x * per;           // seg0 < n_segs: the grid is cdiv(n_segs, per)
#pragma unroll
    for (uint32_t q = 0; q < SORT_TILE / SORT_THREADS; q++) {
        const uint32_t j = threadIdx.x + q * SORT_THREADS, i = j & (P - 1);
        const uint32_t seg = seg0 + j / P;
        const bool live = seg < n_segs && i < n;
        wit_sort_load(cols, k, a, live, (size_t)seg * n + i, i, n, mode, rec, status, key[j], tie[j]);
    }
    for (uint32_t size = 2; size <= P; size <<= 1) wit_sort_lds_strides(key, tie, 0, P - 1, size, size >> 1);
    __syncthreads();                                                      // (P = 1: no stage has run)
    uint32_t wrote = 0;
#pragma unroll
    for (uint32_t q = 0; q < SORT_TILE / SORT_THREADS; q++) {
        const uint32_t j = threadIdx.x + q * SORT_THREADS, i = j & (P - 1);
        const uint32_t seg = seg0 + j / P;
        if (seg < n_segs && i < n && key[(j & ~(P - 1)) + n - 1] != SORT_PAD) {
            st_fe(wit_cell(cols, k, dst[(size_t)seg * n + i]), wit_sort_out<KIND>(key[j], tie[j], n, mode));
            wrote++;
        }
    }
    wit_count(wrote, status);
}

// P > SORT_TILE.  keys: n_segs * P slots of the plan's scratch, segment-major.  Tile kernel: workgroup b loads slots [b * SORT_TILE, + SORT_TILE)
// from the cells, sorts them in LDS through stage SORT_TILE -- in alternating directions: bit SORT_TILE of the place -- and writes the scratch.
__global__ __launch_bounds__(SORT_THREADS) void wit_sort_tile_kernel(WitCols cols, uint32_t k, const uint32_t* __restrict__ a, SortKey* __restrict__ keys, uint32_t n,
                                                                     uint32_t P, uint32_t mode, uint32_t rec, unsigned long long* status) {
    __shared__ int64_t key[SORT_TILE];
    __shared__ uint32_t tie[SORT_TILE];
    const size_t slot0 = (size_t)blockIdx.x * SORT_TILE;                  // the grid is n_segs * P / SORT_TILE
    const uint32_t seg = (uint32_t)(slot0 / P), base = (uint32_t)(slot0 & (P - 1));
#pragma unroll
    for (uint32_t q = 0; q < SORT_TILE / SORT_THREADS; q++) {
        const uint32_t j = threadIdx.x + q * SORT_THREADS, i = base + j;
        wit_sort_load(cols, k, a, i < n, (size_t)seg * n + i, i, n, mode, rec, status, key[j], tie[j]);
    }
    for (uint32_t size = 2; size <= SORT_TILE; size <<= 1) wit_sort_lds_strides(key, tie, base, P - 1, size, size >> 1);
#pragma unroll
    for (uint32_t q = 0; q < SORT_TILE / SORT_THREADS; q++) {
        const uint32_t j = threadIdx.x + q * SORT_THREADS;
        keys[slot0 + j] = SortKey{key[j], tie[j], 0};
    }
}
// one stride >= SORT_TILE of stage `size`: one lane per pair of the n_segs * P / 2 (`pairs`), both keys in the scratch
__global__ __launch_bounds__(SORT_THREADS) void wit_sort_global_kernel(SortKey* __restrict__ keys, size_t pairs, uint32_t P, uint32_t size, uint32_t stride) {
    const size_t t = (size_t)blockIdx.x * SORT_THREADS + threadIdx.x;
    if (t >= pairs) return;
    const size_t i = ((t & ~(size_t)(stride - 1)) << 1) | (t & (stride - 1)), j = i | stride;     // j < 2 * pairs
    const bool asc = (((uint32_t)i & (P - 1)) & size) == 0;
    const SortKey x = keys[i], y = keys[j];
    if (wit_sort_above(x.v, x.tie, y.v, y.tie) == asc) {
        keys[i] = y;
        keys[j] = x;
    }
}
// the strides below SORT_TILE of stage `size` > SORT_TILE: a tile of the scratch through LDS
__global__ __launch_bounds__(SORT_THREADS) void wit_sort_merge_kernel(SortKey* __restrict__ keys, uint32_t P, uint32_t size) {
    __shared__ int64_t key[SORT_TILE];
    __shared__ uint32_t tie[SORT_TILE];
    const size_t slot0 = (size_t)blockIdx.x * SORT_TILE;
#pragma unroll
    for (uint32_t q = 0; q < SORT_TILE / SORT_THREADS; q++) {
        const uint32_t j = threadIdx.x + q * SORT_THREADS;
        const SortKey x = keys[slot0 + j];
        key[j] = x.v; tie[j] = x.tie;
    }
    wit_sort_lds_strides(key, tie, (uint32_t)(slot0 & (P - 1)), P - 1, size, SORT_TILE >> 1);
#pragma unroll
    for (uint32_t q = 0; q < SORT_TILE / SORT_THREADS; q++) {
        const uint32_t j = threadIdx.x + q * SORT_THREADS;
        keys[slot0 + j] = SortKey{key[j], tie[j], 0};
    }
}
// the sorted scratch -> the cells: one lane per destination element
template <uint32_t KIND>
__global__ __launch_bounds__(SORT_THREADS) void wit_sort_store_kernel(WitCols cols, uint32_t k, const uint32_t* __restrict__ dst, const SortKey* __restrict__ keys,
                                                                      uint32_t count, uint32_t n, uint32_t P, uint32_t mode, unsigned long long* status) {
    const uint32_t e = blockIdx.x * SORT_THREADS + threadIdx.x;            // count <= 2^28
    uint32_t wrote = 0;
    if (e < count) {
        const uint32_t seg = e / n, i = e - seg * n;
        const SortKey* s = keys + (size_t)seg * P;
        if (s[n - 1].v != SORT_PAD) {
            const SortKey x = s[i];
            st_fe(wit_cell(cols, k, dst[e]), wit_sort_out<KIND>(x.v, x.tie, n, mode));
            wrote = 1;
        }
    }
    wit_count(wrote, status);
}
EZ_HD uint32_t wit_sort_padded(uint32_t n) {                              // the next power of two: n <= 2^28
    uint32_t P = 1;
    while (P < n) P <<= 1;
    return P;
}

// ARGEXT.  A key is (signed value, position in the segment) with the value negated for argmin (|s| < 2^62: the negation fits), so that both
// modes keep the GREATER value and, at equal values, the SMALLER position: a total order, the combine is associative and commutative, and any
// reduction tree gives the host's answer.  A lane past a segment's end, and a source beyond 62 bits, hold the identity (INT64_MIN, 0xffffffff),
// which no source that fits equals; `bad` -- some source of the segment did not fit -- is carried through the same reduction, so the one
// lane that would store the segment's cell decides not to.  Three regimes by the segment length n: up to 64, 64 / P whole segments to a wave
// (P = the next power of two), log2 P cross-lane steps, no LDS; up to ARGEXT_CHUNK, one workgroup per segment; above, one workgroup per chunk
// into a 16-byte slot of the plan's key scratch (SortKey: v, tie = position, pad = bad), then one workgroup per segment over its slots.
constexpr uint32_t ARGEXT_THREADS = 256, ARGEXT_NO_POS = 0xFFFFFFFFu;
static_assert(ARGEXT_CHUNK % ARGEXT_THREADS == 0 && ARGEXT_THREADS % 64 == 0, "a chunk is whole rounds of a workgroup of whole waves");

// (v, pos, bad) combined with the key (yv, ypos, ybad): the greater value, at equal values the smaller position; bad if either is.  (Three
// scalars on purpose: a struct handed on by reference ends up in the lane's scratch memory.)
EZ_D void wit_argext_take(int64_t& v, uint32_t& pos, uint32_t& bad, int64_t yv, uint32_t ypos, uint32_t ybad) {
    const bool keep = v > yv || (v == yv && pos <= ypos);
    v = keep ? v : yv;
    pos = keep ? pos : ypos;
    bad |= ybad;
}
// the key of source element e = seg * n + i of record `rec` (live: the element exists) combined into (v, pos, bad); reported when it does not fit
EZ_D void wit_argext_load(const WitCols& cols, uint32_t k, const uint32_t* __restrict__ a, bool live, uint32_t e, uint32_t i, uint32_t mode, uint32_t rec,
                          unsigned long long* status, int64_t& v, uint32_t& pos, uint32_t& bad) {
    int64_t yv = INT64_MIN;
    uint32_t ypos = ARGEXT_NO_POS;
    bool fail = false;
    if (live) {
        bool neg, fits;
        uint64_t mag;
        wit_signed(ld_fe(wit_cell(cols, k, a[e])), neg, mag, fits);
        fail = !fits;
        const int64_t s = neg ? -(int64_t)mag : (int64_t)mag;
        yv = fail ? INT64_MIN : mode ? -s : s;
        ypos = fail ? ARGEXT_NO_POS : i;
    }
    wit_report(fail, rec, e, status);
    wit_argext_take(v, pos, bad, yv, ypos, fail ? 1u : 0u);
}
// over aligned groups of `width` lanes (a power of two <= 64): every lane of a group ends with the group's key
EZ_D void wit_argext_lanes(int64_t& v, uint32_t& pos, uint32_t& bad, uint32_t width) {
    for (uint32_t off = width >> 1; off; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, (int)off), hi = (uint32_t)__shfl_xor((int)(uint32_t)((uint64_t)v >> 32), (int)off);
        const uint32_t ypos = (uint32_t)__shfl_xor((int)pos, (int)off), ybad = (uint32_t)__shfl_xor((int)bad, (int)off);
        wit_argext_take(v, pos, bad, (int64_t)((uint64_t)lo | ((uint64_t)hi << 32)), ypos, ybad);
    }
}
// over the workgroup: waves, then the ARGEXT_THREADS / 64 partials through LDS; every lane ends with the workgroup's key
EZ_D void wit_argext_group(int64_t& v, uint32_t& pos, uint32_t& bad, int64_t* part_v, uint32_t* part_pos, uint32_t* part_bad) {
    wit_argext_lanes(v, pos, bad, 64);
    if ((threadIdx.x & 63) == 0) {
        part_v[threadIdx.x >> 6] = v;
        part_pos[threadIdx.x >> 6] = pos;
        part_bad[threadIdx.x >> 6] = bad;
    }
    __syncthreads();
    v = part_v[0]; pos = part_pos[0]; bad = part_bad[0];
#pragma unroll
    for (uint32_t w = 1; w < ARGEXT_THREADS / 64; w++) wit_argext_take(v, pos, bad, part_v[w], part_pos[w], part_bad[w]);
}
// one lane stores a segment's cell unless a source of the segment did not fit
EZ_D void wit_argext_store(const WitCols& cols, uint32_t k, const uint32_t* __restrict__ dst, uint32_t seg, bool mine, uint32_t pos, uint32_t bad, unsigned long long* status) {
    uint32_t wrote = 0;
    if (mine && !bad) {
        st_fe(wit_cell(cols, k, dst[seg]), Fr::from_u64(pos));
        wrote = 1;
    }
    wit_count(wrote, status);
}

// n <= 64: lane l of a wave holds element l % P of the wave's segment l / P; the grid is cdiv(n_segs, (ARGEXT_THREADS / 64) * (64 / P))
__global__ __launch_bounds__(ARGEXT_THREADS) void wit_argext_wave_kernel(WitCols cols, uint32_t k, const uint32_t* __restrict__ dst, const uint32_t* __restrict__ a,
                                                                         uint32_t n_segs, uint32_t n, uint32_t P, uint32_t mode, uint32_t rec, unsigned long long* status) {
    const uint32_t lane = threadIdx.x & 63, wave = blockIdx.x * (ARGEXT_THREADS / 64) + (threadIdx.x >> 6);
    const uint32_t seg = wave * (64 / P) + lane / P, i = lane & (P - 1);
    const bool live = seg < n_segs && i < n;                              // live: seg * n + i < count <= 2^28
    int64_t v = INT64_MIN;
    uint32_t pos = ARGEXT_NO_POS, bad = 0;
    wit_argext_load(cols, k, a, live, seg * n + i, i, mode, rec, status, v, pos, bad);
    wit_argext_lanes(v, pos, bad, P);
    wit_argext_store(cols, k, dst, seg, live && i == 0, pos, bad, status);
}
// n > 64: workgroup b reduces chunk b % chunks -- elements [c * ARGEXT_CHUNK, + ARGEXT_CHUNK) below n -- of segment b / chunks; chunks == 1:
// into the segment's cell, else into slot b of the scratch
__global__ __launch_bounds__(ARGEXT_THREADS) void wit_argext_group_kernel(WitCols cols, uint32_t k, const uint32_t* __restrict__ dst, const uint32_t* __restrict__ a,
                                                                          uint32_t n, uint32_t chunks, uint32_t mode, uint32_t rec, SortKey* __restrict__ slots,
                                                                          unsigned long long* status) {
    __shared__ int64_t part_v[ARGEXT_THREADS / 64];
    __shared__ uint32_t part_pos[ARGEXT_THREADS / 64], part_bad[ARGEXT_THREADS / 64];
    const uint32_t seg = blockIdx.x / chunks, c = blockIdx.x - seg * chunks;
    const uint32_t i0 = c * ARGEXT_CHUNK, i1 = n - i0 < ARGEXT_CHUNK ? n : i0 + ARGEXT_CHUNK;     // i0 < n: chunks = cdiv(n, ARGEXT_CHUNK)
    int64_t v = INT64_MIN;
    uint32_t pos = ARGEXT_NO_POS, bad = 0;
    for (uint32_t base = i0; base < i1; base += ARGEXT_THREADS) {          // the same rounds for every lane: wit_report ballots
        const uint32_t i = base + threadIdx.x;
        wit_argext_load(cols, k, a, i < i1, seg * n + i, i, mode, rec, status, v, pos, bad);
    }
    wit_argext_group(v, pos, bad, part_v, part_pos, part_bad);
    if (chunks > 1) {
        if (threadIdx.x == 0) slots[blockIdx.x] = SortKey{v, pos, bad};
        return;
    }
    wit_argext_store(cols, k, dst, seg, threadIdx.x == 0, pos, bad, status);
}
// the slots of segment blockIdx.x -> its cell
__global__ __launch_bounds__(ARGEXT_THREADS) void wit_argext_final_kernel(WitCols cols, uint32_t k, const uint32_t* __restrict__ dst, const SortKey* __restrict__ slots,
                                                                          uint32_t chunks, unsigned long long* status) {
    __shared__ int64_t part_v[ARGEXT_THREADS / 64];
    __shared__ uint32_t part_pos[ARGEXT_THREADS / 64], part_bad[ARGEXT_THREADS / 64];
    const SortKey* s = slots + (size_t)blockIdx.x * chunks;
    int64_t v = INT64_MIN;
    uint32_t pos = ARGEXT_NO_POS, bad = 0;
    for (uint32_t j = threadIdx.x; j < chunks; j += ARGEXT_THREADS) {
        const SortKey y = s[j];
        wit_argext_take(v, pos, bad, y.v, y.tie, y.pad);
    }
    wit_argext_group(v, pos, bad, part_v, part_pos, part_bad);
    wit_argext_store(cols, k, dst, blockIdx.x, threadIdx.x == 0, pos, bad, status);
}
EZ_HD size_t wit_argext_slots(uint32_t n_segs, uint32_t n) {               // the scratch slots of a record: none unless a segment has several chunks
    const uint32_t chunks = (n + ARGEXT_CHUNK - 1) / ARGEXT_CHUNK;
    return chunks > 1 ? (size_t)n_segs * chunks : 0;
}

// SCATTER.  Element j of the m validates its index s_j -- 0 <= s_j < extent, the test before anything is addressed -- and claims its target
// t_j = s_j * mult + off_j < n (the upload check: off_j + (extent - 1) * mult < n) with atomicMax(winner[t_j], j + 1): the GREATEST element
// on a target wins, whatever the order the lanes arrive in, which is `tensor::ops::scatter`'s "the later element overwrites".  Destination i
// then gets the source cell of element winner[i] - 1, or base cell i where nobody claimed it (the winners start from 0 = nobody; m < 2^31:
// a record's 3m words are in the pool).  A failing element is reported (every one is counted) and raises the record's own failure flag
// -- in LDS or in the scratch, never status[0], which an earlier record may have set -- and the record then stores nothing.
// n <= SCATTER_TILE: one workgroup, the winners in LDS.  Longer: fill, mark and store launches through the plan's scratch: word 0 the
// failure count, the winners from word 4 on.
constexpr uint32_t SCATTER_THREADS = 256, SCATTER_HEAD = 4;
static_assert(SCATTER_TILE % SCATTER_THREADS == 0 && SCATTER_THREADS % 64 == 0 && (SCATTER_TILE / SCATTER_THREADS) <= 32,
              "a tile is whole rounds of a workgroup of whole waves, and a lane's positions of a complement fit a 32-bit mask");

// element j of record `rec` (live: it exists): reported when its index is outside [0, extent); else its winner word is raised to j + 1
EZ_D bool wit_scatter_mark(const WitCols& cols, uint32_t k, const uint32_t* __restrict__ b, uint32_t m, uint32_t mult, bool live, uint32_t j, uint32_t* winner, uint32_t rec,
                           unsigned long long* status) {
    bool fail = false;
    if (live) {
        bool neg, fits;
        uint64_t mag;
        wit_signed(ld_fe(wit_cell(cols, k, b[1 + j])), neg, mag, fits);
        fail = !fits || neg || mag >= b[0];
        if (!fail) atomicMax(&winner[mag * mult + b[1 + 2 * (size_t)m + j]], j + 1);       // < n: checked on upload
    }
    wit_report(fail, rec, j, status);
    return fail;
}
// destination i: the source of the greatest element that claimed it, else its base cell
EZ_D void wit_scatter_put(const WitCols& cols, uint32_t k, const uint32_t* __restrict__ dst, const uint32_t* __restrict__ base, const uint32_t* __restrict__ b, uint32_t m,
                          uint32_t i, uint32_t won) {
    st_fe(wit_cell(cols, k, dst[i]), ld_fe(wit_cell(cols, k, won ? b[1 + m + (won - 1)] : base[i])));
}
__global__ __launch_bounds__(SCATTER_THREADS) void wit_scatter_lds_kernel(WitCols cols, uint32_t k, const uint32_t* __restrict__ dst, const uint32_t* __restrict__ base,
                                                                          const uint32_t* __restrict__ b, uint32_t n, uint32_t m, uint32_t mult, uint32_t rec,
                                                                          unsigned long long* status) {
    __shared__ uint32_t winner[SCATTER_TILE];
    for (uint32_t i = threadIdx.x; i < n; i += SCATTER_THREADS) winner[i] = 0;             // n <= SCATTER_TILE: the launcher's choice
    __syncthreads();
    bool bad = false;
    for (uint32_t j0 = 0; j0 < m; j0 += SCATTER_THREADS)                                  // the same rounds for every lane: wit_report ballots
        bad |= wit_scatter_mark(cols, k, b, m, mult, j0 + threadIdx.x < m, j0 + threadIdx.x, winner, rec, status);
    const bool any_bad = __syncthreads_or(bad ? 1 : 0) != 0;
    uint32_t wrote = 0;
    if (!any_bad)
        for (uint32_t i = threadIdx.x; i < n; i += SCATTER_THREADS, wrote++) wit_scatter_put(cols, k, dst, base, b, m, i, winner[i]);
    wit_count(wrote, status);
}
// the first `head` words zero, the others `value`
__global__ __launch_bounds__(SCATTER_THREADS) void wit_fill_kernel(uint32_t* __restrict__ w, size_t words, uint32_t head, uint32_t value) {
    const size_t i = (size_t)blockIdx.x * SCATTER_THREADS + threadIdx.x;
    if (i < words) w[i] = i < head ? 0u : value;
}
__global__ __launch_bounds__(SCATTER_THREADS) void wit_scatter_mark_kernel(WitCols cols, uint32_t k, const uint32_t* __restrict__ b, uint32_t m, uint32_t mult,
                                                                           uint32_t* __restrict__ scratch, uint32_t rec, unsigned long long* status) {
    const uint32_t j = blockIdx.x * SCATTER_THREADS + threadIdx.x;
    if (wit_scatter_mark(cols, k, b, m, mult, j < m, j, scratch + SCATTER_HEAD, rec, status)) atomicAdd(&scratch[0], 1u);
}
__global__ __launch_bounds__(SCATTER_THREADS) void wit_scatter_store_kernel(WitCols cols, uint32_t k, const uint32_t* __restrict__ dst, const uint32_t* __restrict__ base,
                                                                            const uint32_t* __restrict__ b, uint32_t n, uint32_t m, const uint32_t* __restrict__ scratch,
                                                                            unsigned long long* status) {
    const uint32_t i = blockIdx.x * SCATTER_THREADS + threadIdx.x;
    const bool live = i < n && scratch[0] == 0;
    if (live) wit_scatter_put(cols, k, dst, base, b, m, i, scratch[SCATTER_HEAD + i]);
    wit_count(live ? 1u : 0u, status);
}

// COMPLEMENT.  A source cell whose signed value v lies in [0, n) raises flag v (every writer stores the same 1); the absent v, in ascending
// order, are the destinations: the rank of an absent v is the number of absent values below it -- an exclusive scan -- and v is stored at its
// rank when rank < count (more values than count are absent when sources repeat or lie outside the set: the first `count` are kept).  A
// workgroup resolves SCATTER_TILE values: lane l owns the COMPL_PER consecutive values from l * COMPL_PER on (flag v sits at word v + v / 32 of
// the LDS array, so that the lanes' strided reads fall on distinct banks), counts its absent ones, the counts are scanned with cross-lane steps
// within a wave and through LDS across the waves, and the lane walks its values again.  n <= SCATTER_TILE: one launch.  Longer sets: the
// flags are bytes of the plan's scratch (fill, mark), a launch leaves every workgroup's absent count behind them, one workgroup turns the
// counts into offsets -- looping when there are more workgroups than lanes --, and a launch compacts.
constexpr uint32_t COMPL_PER = SCATTER_TILE / SCATTER_THREADS, COMPL_WORDS = SCATTER_TILE + SCATTER_TILE / 32;
EZ_D uint32_t wit_compl_at(uint32_t v) { return v + (v >> 5); }
// the flag a source raises: its signed value when that lies in [0, n), else none (n itself)
EZ_D uint32_t wit_compl_value(const WitCols& cols, uint32_t k, uint32_t cell, uint32_t n) {
    bool neg, fits;
    uint64_t mag;
    wit_signed(ld_fe(wit_cell(cols, k, cell)), neg, mag, fits);
    return fits && !neg && mag < n ? (uint32_t)mag : n;
}
// the exclusive scan of c over the workgroup (every lane calls it); total: the workgroup's sum.  part: SCATTER_THREADS / 64 words of LDS
EZ_D uint32_t wit_compl_scan(uint32_t c, uint32_t* part, uint32_t& total) {
    uint32_t incl = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)incl, off);
        if ((threadIdx.x & 63) >= (uint32_t)off) incl += o;
    }
    __syncthreads();                                                      // (part may still be read from an earlier call)
    if ((threadIdx.x & 63) == 63) part[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (uint32_t w = 0; w < SCATTER_THREADS / 64; w++) {
        before += w < (threadIdx.x >> 6) ? part[w] : 0;
        total += part[w];
    }
    return before + incl - c;
}
// the values [v0, v0 + SCATTER_TILE) below n with their flags in LDS: absent v -> dst[rank] while rank < count, rank = offset + the absent below v
// in the tile; STORE false: only the tile's absent count is returned
template <bool STORE>
EZ_D uint32_t wit_compl_tile(const WitCols& cols, uint32_t k, const uint32_t* __restrict__ dst, const uint32_t* flag, uint32_t* part, uint32_t v0, uint32_t n,
                             uint32_t offset, uint32_t count, uint32_t& wrote) {
    uint32_t absent = 0;
#pragma unroll
    for (uint32_t q = 0; q < COMPL_PER; q++) {
        const uint32_t t = threadIdx.x * COMPL_PER + q;
        absent |= (t < n - v0 && !flag[wit_compl_at(t)] ? 1u : 0u) << q;                   // v0 < n: a tile starts inside the set
    }
    uint32_t total;
    uint32_t rank = offset + wit_compl_scan(__popc(absent), part, total);
    if (STORE)
        for (uint32_t q = 0; q < COMPL_PER; q++)
            if ((absent >> q) & 1) {
                if (rank < count) {
                    st_fe(wit_cell(cols, k, dst[rank]), Fr::from_u64(v0 + threadIdx.x * COMPL_PER + q));
                    wrote++;
                }
                rank++;
            }
    return total;
}
__global__ __launch_bounds__(SCATTER_THREADS) void wit_compl_lds_kernel(WitCols cols, uint32_t k, const uint32_t* __restrict__ dst, const uint32_t* __restrict__ a,
                                                                        uint32_t n, uint32_t m, uint32_t count, unsigned long long* status) {
    __shared__ uint32_t flag[COMPL_WORDS], part[SCATTER_THREADS / 64];
    for (uint32_t i = threadIdx.x; i < COMPL_WORDS; i += SCATTER_THREADS) flag[i] = 0;
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < m; j += SCATTER_THREADS) {
        const uint32_t v = wit_compl_value(cols, k, a[j], n);
        if (v < n) flag[wit_compl_at(v)] = 1;                                             // n <= SCATTER_TILE: the launcher's choice
    }
    __syncthreads();
    uint32_t wrote = 0;
    wit_compl_tile<true>(cols, k, dst, flag, part, 0, n, 0, count, wrote);
    wit_count(wrote, status);
}
__global__ __launch_bounds__(SCATTER_THREADS) void wit_compl_mark_kernel(WitCols cols, uint32_t k, const uint32_t* __restrict__ a, uint32_t n, uint32_t m,
                                                                         uint8_t* __restrict__ flags) {
    const uint32_t j = blockIdx.x * SCATTER_THREADS + threadIdx.x;
    if (j >= m) return;
    const uint32_t v = wit_compl_value(cols, k, a[j], n);
    if (v < n) flags[v] = 1;
}
// workgroup b over the values [b * SCATTER_TILE, + SCATTER_TILE): STORE false -> counts[b] = its absent count; true -> compacted from the offset counts[b]
template <bool STORE>
__global__ __launch_bounds__(SCATTER_THREADS) void wit_compl_tile_kernel(WitCols cols, uint32_t k, const uint32_t* __restrict__ dst, const uint8_t* __restrict__ flags,
                                                                         uint32_t* __restrict__ counts, uint32_t n, uint32_t count, unsigned long long* status) {
    __shared__ uint32_t flag[COMPL_WORDS], part[SCATTER_THREADS / 64];
    const uint32_t v0 = blockIdx.x * SCATTER_TILE;                                        // < n: the grid is cdiv(n, SCATTER_TILE)
    for (uint32_t t = threadIdx.x; t < SCATTER_TILE; t += SCATTER_THREADS) flag[wit_compl_at(t)] = t < n - v0 ? flags[v0 + t] : 1u;
    __syncthreads();
    uint32_t wrote = 0;
    const uint32_t total = wit_compl_tile<STORE>(cols, k, dst, flag, part, v0, n, STORE ? counts[blockIdx.x] : 0u, count, wrote);
    if (!STORE && threadIdx.x == 0) counts[blockIdx.x] = total;
    if (STORE) wit_count(wrote, status);
}
// counts[0 .. blocks) -> their exclusive prefix sums, in place: one workgroup, SCATTER_THREADS counts a round with the running total carried on
__global__ __launch_bounds__(SCATTER_THREADS) void wit_compl_offsets_kernel(uint32_t* __restrict__ counts, uint32_t blocks) {
    __shared__ uint32_t part[SCATTER_THREADS / 64];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < blocks; base += SCATTER_THREADS) {                      // the same rounds for every lane: the scan has barriers
        const uint32_t i = base + threadIdx.x;
        uint32_t total;
        const uint32_t before = wit_compl_scan(i < blocks ? counts[i] : 0u, part, total);
        if (i < blocks) counts[i] = carry + before;
        carry += total;
    }
}
EZ_HD size_t wit_compl_flag_bytes(uint32_t n) { return ((size_t)n + 15) / 16 * 16; }       // the counts follow the flags, aligned
// the scratch bytes of a SCATTER / COMPLEMENT record: none while one workgroup holds it in LDS
EZ_HD size_t wit_scatter_scratch(const Rec& r) {
    if (r.kind == SCATTER) return r.count > SCATTER_TILE ? ((size_t)r.count + SCATTER_HEAD) * 4 : 0;
    if (r.kind == COMPLEMENT) return r.p0 > SCATTER_TILE ? wit_compl_flag_bytes(r.p0) + (((size_t)r.p0 + SCATTER_TILE - 1) / SCATTER_TILE) * 4 : 0;
    return 0;
}

struct DevPlan {
    Plan host;                      // the validated blob: records, outputs and counts drive the launches; pool / params / consts are
                                    // released once they are on the device (n_params is kept for ezkl_hip_witness_plan_info)
    uint32_t n_params = 0;
    uint32_t* pool = nullptr;       // device copies, read-only after upload
    uint32_t* outputs = nullptr;
    int64_t* params = nullptr;
    fe_t* consts = nullptr;         // Montgomery form
    int64_t* table_values = nullptr;   // the static lookup tables' values (directory: host.tables)
    // per-run scratch, owned by the plan (from the column pool: nothing is allocated per run)
    int64_t* inputs = nullptr;
    fe_t* outs = nullptr;
    unsigned long long* status = nullptr;
    SortKey* sort_keys = nullptr;   // the padded keys of the largest sort record with segments above SORT_TILE, or the chunk slots of the
                                    // largest arg-extremum record with segments above ARGEXT_CHUNK, or the winner words / the flags and counts of the
                                    // largest scatter / complement record above SCATTER_TILE, whichever is more (one slot when there is none)
    StatRec* stat_recs = nullptr;   // (source offset, count) of every TABLE record, in all phases: what ezkl_hip_witness_lookup_stats_dev strides over
    uint32_t n_stat_recs = 0;
    uint64_t stat_elems = 0;
    long long* stats = nullptr;     // its result words: least, greatest, sources beyond 62 bits; set per call
    Ctx* ctx = nullptr;
    // a plan with phases: the last phase that ran to its end since the last phase 0 with no earlier phase started again since, and the
    // columns it ran on
    int done_phase = -1;
    void* done_cols[MAX_ADVICE] = {nullptr};
};
thread_local std::string t_wit_error;
std::atomic<uint64_t> g_wide_dots{0};                             // DOT records launched on wit_dot_wide_kernel (ezkl_hip_witness_wide_dots)
// the bytes of sort_keys a record's launchers go through
size_t wit_scratch_bytes(const Rec& r) {
    if (r.kind == SORT || r.kind == ARGSORT)                      // segments * P * 16 B of a sort that leaves LDS
        return wit_sort_padded(r.p0) > SORT_TILE ? (size_t)(r.count / r.p0) * wit_sort_padded(r.p0) * sizeof(SortKey) : 0;
    if (r.kind == ARGEXT) return wit_argext_slots(r.count, r.p0) * sizeof(SortKey);
    return wit_scatter_scratch(r);                                // SCATTER, COMPLEMENT; every other kind: none
}

void plan_release(DevPlan* p) {
    for (void* q : {(void*)p->pool, (void*)p->outputs, (void*)p->params, (void*)p->consts, (void*)p->table_values, (void*)p->inputs, (void*)p->outs, (void*)p->status, (void*)p->sort_keys, (void*)p->stat_recs, (void*)p->stats})
        if (q) (void)ezkl_hip_free(q);
    delete p;
}
template <uint32_t KIND>
void launch_elem(hipStream_t st, const WitCols& cols, uint32_t k, const DevPlan* p, const Rec& r, uint32_t ri) {
    const int64_t* ints = KIND == INPUT ? p->inputs : p->params;
    uint32_t p0 = r.p0, p1 = r.p1, p2 = 0;
    if (KIND == TABLE || KIND == TBLIDX) {                            // the directory entry, resolved here: r.p0 < tables.size() was checked on upload
        const Table& t = p->host.tables[r.p0];
        ints = p->table_values + t.off;
        p0 = (uint32_t)t.lo; p1 = t.n; p2 = t.col_size;
    }
    if (KIND == RECIP) p2 = r.b;                                      // the constant a zero input takes: r.b < the constants, checked on upload
    const uint32_t* b = p->pool + (KIND == GATHER ? r.p0 : KIND == RECIP ? 0 : r.b);     // GATHER: the table's cell list, inside the pool: checked on upload
    hipLaunchKernelGGL(wit_elem_kernel<KIND>, dim3(cdiv(r.count, 256)), dim3(256), 0, st, cols, k, p->pool + r.dst, p->pool + r.a, b, r.count, p0, p1, p2,
                       ints, (const fe_t*)p->consts, ri, p->status);
}
// a SORT / ARGSORT record: one launch when a padded segment fits a tile, else tile sort, per stage the strides at or above the tile one launch
// each and one for those below it, store.  -> the number of launches
template <uint32_t KIND>
uint32_t launch_sort(hipStream_t st, const WitCols& cols, uint32_t k, const DevPlan* p, const Rec& r, uint32_t ri) {
    const uint32_t n = r.p0, n_segs = r.count / n, P = wit_sort_padded(n);
    if (P <= SORT_TILE) {
        hipLaunchKernelGGL(wit_sort_lds_kernel<KIND>, dim3(cdiv(n_segs, SORT_TILE / P)), dim3(SORT_THREADS), 0, st, cols, k, p->pool + r.dst, p->pool + r.a, n_segs, n, P, r.p1, ri,
                           p->status);
        return 1;
    }
    const size_t slots = (size_t)n_segs * P;                             // <= 2^29: count <= 2^28 and P < 2 n
    const uint32_t tiles = (uint32_t)(slots / SORT_TILE);
    uint32_t launches = 2;
    hipLaunchKernelGGL(wit_sort_tile_kernel, dim3(tiles), dim3(SORT_THREADS), 0, st, cols, k, p->pool + r.a, p->sort_keys, n, P, r.p1, ri, p->status);
    for (uint32_t size = 2 * SORT_TILE; size <= P; size <<= 1) {
        for (uint32_t stride = size >> 1; stride >= SORT_TILE; stride >>= 1, launches++)
            hipLaunchKernelGGL(wit_sort_global_kernel, dim3((uint32_t)cdiv(slots / 2, SORT_THREADS)), dim3(SORT_THREADS), 0, st, p->sort_keys, slots / 2, P, size, stride);
        hipLaunchKernelGGL(wit_sort_merge_kernel, dim3(tiles), dim3(SORT_THREADS), 0, st, p->sort_keys, P, size);
        launches++;
    }
    hipLaunchKernelGGL(wit_sort_store_kernel<KIND>, dim3(cdiv(r.count, SORT_THREADS)), dim3(SORT_THREADS), 0, st, cols, k, p->pool + r.dst, (const SortKey*)p->sort_keys, r.count, n, P,
                       r.p1, p->status);
    return launches;
}
// an ARGEXT record: one launch up to ARGEXT_CHUNK sources a segment, else the chunks into the scratch and the slots into the cells.  -> the
// number of launches
uint32_t launch_argext(hipStream_t st, const WitCols& cols, uint32_t k, const DevPlan* p, const Rec& r, uint32_t ri) {
    const uint32_t n = r.p0, n_segs = r.count;                           // n_segs * n <= 2^28, checked on upload
    if (n <= 64) {
        const uint32_t P = wit_sort_padded(n);
        hipLaunchKernelGGL(wit_argext_wave_kernel, dim3(cdiv(n_segs, (ARGEXT_THREADS / 64) * (64 / P))), dim3(ARGEXT_THREADS), 0, st, cols, k, p->pool + r.dst, p->pool + r.a, n_segs,
                           n, P, r.p1, ri, p->status);
        return 1;
    }
    const uint32_t chunks = cdiv(n, ARGEXT_CHUNK);                       // n_segs * chunks <= 2^28 / ARGEXT_CHUNK + n_segs
    hipLaunchKernelGGL(wit_argext_group_kernel, dim3(n_segs * chunks), dim3(ARGEXT_THREADS), 0, st, cols, k, p->pool + r.dst, p->pool + r.a, n, chunks, r.p1, ri, p->sort_keys,
                       p->status);
    if (chunks == 1) return 1;
    hipLaunchKernelGGL(wit_argext_final_kernel, dim3(n_segs), dim3(ARGEXT_THREADS), 0, st, cols, k, p->pool + r.dst, (const SortKey*)p->sort_keys, chunks, p->status);
    return 2;
}
// a SCATTER record: one launch up to SCATTER_TILE destinations, else fill, mark and store through the scratch.  -> the number of launches
uint32_t launch_scatter(hipStream_t st, const WitCols& cols, uint32_t k, const DevPlan* p, const Rec& r, uint32_t ri) {
    const uint32_t n = r.count, m = r.p0;                                // n <= 2^28, m >= 1: checked on upload
    const uint32_t *dst = p->pool + r.dst, *base = p->pool + r.a, *b = p->pool + r.b;
    if (n <= SCATTER_TILE) {
        hipLaunchKernelGGL(wit_scatter_lds_kernel, dim3(1), dim3(SCATTER_THREADS), 0, st, cols, k, dst, base, b, n, m, r.p1, ri, p->status);
        return 1;
    }
    uint32_t* scratch = reinterpret_cast<uint32_t*>(p->sort_keys);        // SCATTER_HEAD + n words: sized on upload
    hipLaunchKernelGGL(wit_fill_kernel, dim3((uint32_t)cdiv((size_t)n + SCATTER_HEAD, SCATTER_THREADS)), dim3(SCATTER_THREADS), 0, st, scratch, (size_t)n + SCATTER_HEAD, SCATTER_HEAD, 0u);
    hipLaunchKernelGGL(wit_scatter_mark_kernel, dim3(cdiv(m, SCATTER_THREADS)), dim3(SCATTER_THREADS), 0, st, cols, k, b, m, r.p1, scratch, ri, p->status);
    hipLaunchKernelGGL(wit_scatter_store_kernel, dim3(cdiv(n, SCATTER_THREADS)), dim3(SCATTER_THREADS), 0, st, cols, k, dst, base, b, n, m, (const uint32_t*)scratch, p->status);
    return 3;
}
// a COMPLEMENT record: none when it has no cell, one launch up to SCATTER_TILE values, else fill, mark, count, offsets and compact through the
// scratch.  -> the number of launches
uint32_t launch_complement(hipStream_t st, const WitCols& cols, uint32_t k, const DevPlan* p, const Rec& r) {
    const uint32_t n = r.p0, m = r.p1, count = r.count;                  // m <= n <= 2^28, count = n - m: checked on upload
    if (count == 0) return 0;
    const uint32_t *dst = p->pool + r.dst, *a = p->pool + r.a;
    if (n <= SCATTER_TILE) {
        hipLaunchKernelGGL(wit_compl_lds_kernel, dim3(1), dim3(SCATTER_THREADS), 0, st, cols, k, dst, a, n, m, count, p->status);
        return 1;
    }
    uint8_t* flags = reinterpret_cast<uint8_t*>(p->sort_keys);            // the flag bytes, then one count per tile: sized on upload
    uint32_t* counts = reinterpret_cast<uint32_t*>(flags + wit_compl_flag_bytes(n));
    const uint32_t blocks = cdiv(n, SCATTER_TILE);
    const size_t words = wit_compl_flag_bytes(n) / 4;
    uint32_t launches = 4;
    hipLaunchKernelGGL(wit_fill_kernel, dim3((uint32_t)cdiv(words, SCATTER_THREADS)), dim3(SCATTER_THREADS), 0, st, reinterpret_cast<uint32_t*>(flags), words, 0u, 0u);
    if (m) {
        hipLaunchKernelGGL(wit_compl_mark_kernel, dim3(cdiv(m, SCATTER_THREADS)), dim3(SCATTER_THREADS), 0, st, cols, k, a, n, m, flags);
        launches++;
    }
    hipLaunchKernelGGL(wit_compl_tile_kernel<false>, dim3(blocks), dim3(SCATTER_THREADS), 0, st, cols, k, dst, (const uint8_t*)flags, counts, n, count, p->status);
    hipLaunchKernelGGL(wit_compl_offsets_kernel, dim3(1), dim3(SCATTER_THREADS), 0, st, counts, blocks);
    hipLaunchKernelGGL(wit_compl_tile_kernel<true>, dim3(blocks), dim3(SCATTER_THREADS), 0, st, cols, k, dst, (const uint8_t*)flags, counts, n, count, p->status);
    return launches;
}
}  // namespace
}  // namespace ezkl

using namespace ezkl;

extern "C" {

const char* ezkl_hip_witness_last_error(void) { return t_wit_error.c_str(); }

int ezkl_hip_witness_wide_dots(uint64_t* launches, int reset) {
    if (!launches) return EZKL_ERR_INVALID;
    *launches = reset ? g_wide_dots.exchange(0) : g_wide_dots.load();
    return EZKL_OK;
}

int ezkl_hip_witness_plan_upload(const void* blob, size_t len, ezkl_wplan_t* out) {
    if (!out) return EZKL_ERR_INVALID;
    *out = nullptr;
    DevPlan* p = new DevPlan();
    if (!wplan::parse(blob, len, p->host, t_wit_error)) {          // host-only: a bad blob is refused before a device is asked for
        delete p;
        return EZKL_ERR_INVALID;
    }
    t_wit_error.clear();
    Ctx* c = ctx();
    if (!c) { delete p; return EZKL_ERR_NO_DEVICE; }
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    p->ctx = c;
    const Plan& h = p->host;
    std::vector<fe_t> consts(h.consts.size() / 32);
    for (size_t i = 0; i < consts.size(); i++) {
        fe_t v;
        memcpy(v.v, h.consts.data() + 32 * i, 32);
        consts[i] = Fr::to_mont(v);
    }
    size_t sort_bytes = 0;                                        // the records run one after another on the stream: they share the scratch
    for (const Rec& r : h.recs) sort_bytes = std::max(sort_bytes, wit_scratch_bytes(r));
    std::vector<StatRec> stat_recs;
    for (const Rec& r : h.recs)
        if (r.kind == TABLE) {
            stat_recs.push_back(StatRec{r.a, r.count});
            p->stat_elems += r.count;
        }
    p->n_stat_recs = (uint32_t)stat_recs.size();
    struct Up { void** dev; const void* src; size_t bytes; };
    const Up ups[] = {{(void**)&p->pool, h.pool.data(), h.pool.size() * 4},       {(void**)&p->outputs, h.outputs.data(), h.outputs.size() * 4},
                      {(void**)&p->params, h.params.data(), h.params.size() * 8}, {(void**)&p->consts, consts.data(), consts.size() * 32},
                      {(void**)&p->inputs, nullptr, (size_t)h.n_inputs * 8},      {(void**)&p->outs, nullptr, h.outputs.size() * 32},
                      {(void**)&p->status, nullptr, 32},                          {(void**)&p->table_values, h.table_values.data(), h.table_values.size() * 8},
                      {(void**)&p->sort_keys, nullptr, sort_bytes},               {(void**)&p->stat_recs, stat_recs.data(), stat_recs.size() * sizeof(StatRec)},
                      {(void**)&p->stats, nullptr, 32}};
    int rc = EZKL_OK;
    for (const Up& u : ups) {
        if ((rc = ezkl_hip_malloc(u.dev, u.bytes ? u.bytes : 1))) break;
        if (u.src && u.bytes && (rc = ezkl_hip_memcpy_h2d(*u.dev, u.src, u.bytes))) break;
    }
    if (!rc) rc = ezkl_hip_synchronize();
    if (rc) { plan_release(p); return rc; }
    p->n_params = (uint32_t)h.params.size();
    std::vector<uint32_t>().swap(p->host.pool);                   // 138 MB at k = 20: the device copy is the one that is read from here on
    std::vector<int64_t>().swap(p->host.params);
    std::vector<uint8_t>().swap(p->host.consts);
    std::vector<int64_t>().swap(p->host.table_values);            // (the directory stays: the launcher resolves it)
    *out = reinterpret_cast<ezkl_wplan_t>(p);
    return EZKL_OK;
}

int ezkl_hip_witness_plan_free(ezkl_wplan_t plan) {
    if (!plan) return EZKL_OK;
    DevPlan* p = reinterpret_cast<DevPlan*>(plan);
    EZ_CTX(c);
    if (c != p->ctx) return EZKL_ERR_INVALID;
    EZ_HIP(hipStreamSynchronize(c->stream));
    plan_release(p);
    return EZKL_OK;
}

int ezkl_hip_witness_plan_info(ezkl_wplan_t plan, uint32_t out[8]) {
    if (!plan || !out) return EZKL_ERR_INVALID;
    const Plan& h = reinterpret_cast<DevPlan*>(plan)->host;
    const uint32_t v[8] = {h.k, h.n_advice, h.n_inputs, (uint32_t)h.outputs.size(), (uint32_t)h.recs.size(), h.n_cells, h.n_ops, reinterpret_cast<DevPlan*>(plan)->n_params};
    memcpy(out, v, sizeof v);
    return EZKL_OK;
}

int ezkl_hip_witness_plan_phases(ezkl_wplan_t plan, uint32_t out[2], uint8_t* column_phase) {
    if (!plan || !out) return EZKL_ERR_INVALID;
    const Plan& h = reinterpret_cast<DevPlan*>(plan)->host;
    out[0] = h.n_phases; out[1] = h.n_challenges;
    if (column_phase) memcpy(column_phase, h.col_phase, h.n_advice);
    return EZKL_OK;
}

int ezkl_hip_witness_run_phase_dev(ezkl_wplan_t plan, uint32_t phase, const int64_t* inputs_host, size_t n_inputs, const void* challenges, size_t n_challenges,
                                   void* const* advice_cols_dev, void* outputs_host, uint64_t status[4], void* stream) {
    if (!plan || !advice_cols_dev || !status) return EZKL_ERR_INVALID;
    memset(status, 0, 4 * sizeof(uint64_t));
    t_wit_error.clear();
    DevPlan* p = reinterpret_cast<DevPlan*>(plan);
    const Plan& h = p->host;
    const bool first = phase == 0, last = phase + 1 == h.n_phases;
    auto refuse = [&](const char* why) { t_wit_error = std::string("witness: ") + why; return EZKL_ERR_INVALID; };
    if (phase >= h.n_phases) return refuse("no such phase");
    if (first && (n_inputs != h.n_inputs || (n_inputs && !inputs_host))) return refuse("the inputs go with phase 0, all of them");
    if (last && !h.outputs.empty() && !outputs_host) return EZKL_ERR_INVALID;
    if (n_challenges && !challenges) return EZKL_ERR_INVALID;
    WitCols cols;
    for (uint32_t j = 0; j < MAX_ADVICE; j++) cols.p[j] = nullptr;
    for (uint32_t j = 0; j < h.n_advice; j++) {
        if (!advice_cols_dev[j]) return EZKL_ERR_INVALID;
        for (uint32_t i = 0; i < j; i++)
            if (advice_cols_dev[i] == advice_cols_dev[j]) return EZKL_ERR_INVALID;
        cols.p[j] = static_cast<fe_t*>(advice_cols_dev[j]);
    }
    // the challenges: canonical -> Montgomery here, handed to the kernels by value
    std::vector<fe_t> chal(n_challenges);
    for (size_t i = 0; i < n_challenges; i++) {
        const uint8_t* c = static_cast<const uint8_t*>(challenges) + 32 * i;
        if (!wplan::canonical(c)) return refuse("a challenge is not a canonical field element");
        fe_t v;
        memcpy(v.v, c, 32);
        chal[i] = Fr::to_mont(v);
    }
    for (const Rec& r : h.recs)
        if (r.phase == phase && r.kind == RLC && r.p0 >= n_challenges) return refuse("the phase reads a challenge that was not passed");
    if (first) p->done_phase = -1;
    else {                                                     // the cells of the earlier phases must be where this one reads them
        bool same = p->done_phase >= (int)phase - 1;
        for (uint32_t j = 0; same && j < h.n_advice; j++) same = p->done_cols[j] == advice_cols_dev[j];
        if (!same) return refuse(("phase " + std::to_string(phase) + " before phase " + std::to_string(phase - 1) + " on these columns").c_str());
        // this run zero-fills and rewrites the columns of its phase: until it has finished clean nothing later may read them, whatever an
        // earlier run of this phase or a later one had finished
        p->done_phase = (int)phase - 1;
    }
    EZ_CTX(c);
    if (c != p->ctx) return EZKL_ERR_INVALID;
    hipStream_t st = pick_stream(c, stream);
    const uint32_t k = h.k;
    const size_t n = (size_t)1 << k;
    uint64_t launches = 0;
    hipEvent_t e0, e1;
    int rc = ev_pair(c, "witness", &e0, &e1);
    if (rc) return rc;
    EZ_HIP(hipEventRecord(e0, st));
    for (uint32_t j = 0; j < h.n_advice; j++)                  // the columns of this phase only: the earlier phases' cells stay
        if (h.col_phase[j] == phase) {
            EZ_HIP(hipMemsetAsync(cols.p[j], 0, n * sizeof(fe_t), st));
            launches++;
        }
    EZ_HIP(hipMemsetAsync(p->status, 0, 32, st));
    launches++;
    if (first && n_inputs) EZ_HIP(hipMemcpyAsync(p->inputs, inputs_host, n_inputs * 8, hipMemcpyHostToDevice, st));
    for (size_t ri = 0; ri < h.recs.size(); ri++) {
        const Rec& r = h.recs[ri];
        if (r.phase != phase) continue;
        switch (r.kind) {
#define EZ_WIT_ELEM(KIND) case KIND: launch_elem<KIND>(st, cols, k, p, r, (uint32_t)ri); break;
        EZ_WIT_ELEM(COPY) EZ_WIT_ELEM(CONST) EZ_WIT_ELEM(INPUT) EZ_WIT_ELEM(PARAM) EZ_WIT_ELEM(ADD) EZ_WIT_ELEM(SUB) EZ_WIT_ELEM(MUL) EZ_WIT_ELEM(HINT) EZ_WIT_ELEM(RCIDX)
        EZ_WIT_ELEM(INVZ) EZ_WIT_ELEM(TABLE) EZ_WIT_ELEM(TBLIDX) EZ_WIT_ELEM(DIVC) EZ_WIT_ELEM(GATHER) EZ_WIT_ELEM(CLAMP) EZ_WIT_ELEM(RECIP) EZ_WIT_ELEM(ISQRT)
        case SUMACC:
            hipLaunchKernelGGL(wit_acc_kernel<SUMACC>, dim3(cdiv((size_t)r.count * DOT_LANES, 64)), dim3(64), 0, st, cols, k, p->pool + r.dst, p->pool + r.a, r.count, r.p0, r.p1,
                               p->status);
            break;
        case PRODACC:
            hipLaunchKernelGGL(wit_acc_kernel<PRODACC>, dim3(cdiv((size_t)r.count * DOT_LANES, 64)), dim3(64), 0, st, cols, k, p->pool + r.dst, p->pool + r.a, r.count, r.p0, r.p1,
                               p->status);
            break;
        case SORT: launches += launch_sort<SORT>(st, cols, k, p, r, (uint32_t)ri) - 1; break;
        case ARGSORT: launches += launch_sort<ARGSORT>(st, cols, k, p, r, (uint32_t)ri) - 1; break;
        case ARGEXT: launches += launch_argext(st, cols, k, p, r, (uint32_t)ri) - 1; break;
        EZ_WIT_ELEM(ONEHOT)                                        // (here, not above: the kernels are emitted in the order of their first use)
#undef EZ_WIT_ELEM
        case SCATTER: launches += launch_scatter(st, cols, k, p, r, (uint32_t)ri) - 1; break;
        case COMPLEMENT: {
            const uint32_t made = launch_complement(st, cols, k, p, r);
            if (!made) continue;                                   // nothing missing: the record writes no cell
            launches += made - 1;
            break;
        }
        case MATMUL: {
            const uint32_t m = r.count / r.p1;
            hipLaunchKernelGGL(wit_matmul_kernel, dim3(cdiv(m, MM_TILE) * cdiv(r.p1, MM_TILE)), dim3(MM_TILE * MM_TILE), 0, st, cols, k, p->pool + r.dst, p->pool + r.a,
                               p->pool + r.b, m, r.p0, r.p1, (const int64_t*)p->inputs, (uint32_t)ri, p->status);
            break;
        }
        case RLC:
            hipLaunchKernelGGL(wit_rlc_kernel, dim3(cdiv((size_t)r.count * RLC_LANES, 64)), dim3(64), 0, st, cols, k, p->pool + r.dst, p->pool + r.a, r.count, r.p1, chal[r.p0],
                               p->status);
            break;
        case DOT:
            if (r.p1 == 1 && r.p0 >= DOT_WIDE_MIN) {                 // one long step: every lane multiplies
                const uint32_t lanes = dot_wide_lanes(r.count, r.p0);
                hipLaunchKernelGGL(wit_dot_wide_kernel, dim3(cdiv((size_t)r.count, 64 / lanes)), dim3(64), 0, st, cols, k, p->pool + r.dst, p->pool + r.a, p->pool + r.b,
                                   r.count, r.p0, lanes, p->status);
                g_wide_dots.fetch_add(1, std::memory_order_relaxed);
                break;
            }
            hipLaunchKernelGGL(wit_dot_kernel,dim3(cdiv((size_t)r.count * DOT_LANES, 64)), dim3(64), 0, st, cols, k, p->pool + r.dst, p->pool + r.a, p->pool + r.b, r.count, r.p0, r.p1,
                               p->status);
            break;
        default:                                                   // (`parse` refuses every kind this loop does not name)
            t_wit_error = "witness: unhandled record kind " + std::to_string(r.kind);
            return EZKL_ERR_INVALID;
        }
        EZ_HIP(hipGetLastError());
        launches++;
    }
    const bool gather = last && !h.outputs.empty();
    if (gather) {
        hipLaunchKernelGGL(wit_gather_kernel, dim3(cdiv(h.outputs.size(), 64)), dim3(64), 0, st, cols, k, p->outputs, (uint32_t)h.outputs.size(), p->outs);
        EZ_HIP(hipGetLastError());
        launches++;
    }
    EZ_HIP(hipEventRecord(e1, st));
    unsigned long long dev_status[4] = {0, 0, 0, 0};
    if (gather) EZ_HIP(hipMemcpyAsync(outputs_host, p->outs, h.outputs.size() * 32, hipMemcpyDeviceToHost, st));
    EZ_HIP(hipMemcpyAsync(dev_status, p->status, 32, hipMemcpyDeviceToHost, st));
    EZ_HIP(hipStreamSynchronize(st));
    status[0] = dev_status[0];
    status[1] = dev_status[0] ? ~dev_status[1] : 0;
    status[2] = dev_status[2];
    status[3] = launches;
    if (dev_status[0]) {
        const uint32_t ri = (uint32_t)(status[1] >> 32), el = (uint32_t)status[1];
        const uint32_t kind = ri < h.recs.size() ? h.recs[ri].kind : (uint32_t)KINDS_TOP;     // (KINDS_TOP: no such record)
        t_wit_error = std::string("witness: ") + failure_words(kind) + " (" + kind_name(kind) + " record " + std::to_string(ri) + ", element " + std::to_string(el) + "; " +
                      std::to_string(dev_status[0]) + " " + (kind < KINDS_TOP ? KINDS[kind].unit : "cells") + " in all)";
        return EZKL_ERR_INVALID;
    }
    p->done_phase = (int)phase;
    if (first) memcpy(p->done_cols, advice_cols_dev, h.n_advice * sizeof(void*));
    t_wit_error.clear();
    return EZKL_OK;
}

int ezkl_hip_witness_lookup_stats_dev(ezkl_wplan_t plan, void* const* advice_cols_dev, int64_t out_min_max[2], void* stream) {
    if (!plan || !advice_cols_dev || !out_min_max) return EZKL_ERR_INVALID;
    out_min_max[0] = out_min_max[1] = 0;
    t_wit_error.clear();
    DevPlan* p = reinterpret_cast<DevPlan*>(plan);
    const Plan& h = p->host;
    WitCols cols;
    for (uint32_t j = 0; j < MAX_ADVICE; j++) cols.p[j] = nullptr;
    for (uint32_t j = 0; j < h.n_advice; j++) {
        if (!advice_cols_dev[j]) return EZKL_ERR_INVALID;
        cols.p[j] = static_cast<fe_t*>(advice_cols_dev[j]);
    }
    if (p->n_stat_recs == 0) return EZKL_OK;                       // no static lookup: (0, 0), nothing launched
    EZ_CTX(c);
    if (c != p->ctx) return EZKL_ERR_INVALID;
    hipStream_t st = pick_stream(c, stream);
    hipEvent_t e0, e1;
    int rc = ev_pair(c, "witness_lookup_stats", &e0, &e1);
    if (rc) return rc;
    const uint64_t blocks = (p->stat_elems + STATS_THREADS - 1) / STATS_THREADS;
    EZ_HIP(hipEventRecord(e0, st));
    EZ_HIP(hipMemsetAsync(p->stats, 0, 32, st));
    hipLaunchKernelGGL(wit_lookup_stats_kernel, dim3((uint32_t)(blocks < STATS_MAX_BLOCKS ? blocks : STATS_MAX_BLOCKS)), dim3(STATS_THREADS), 0, st, cols, h.k,
                       (const uint32_t*)p->pool, (const StatRec*)p->stat_recs, p->n_stat_recs, p->stats);
    EZ_HIP(hipGetLastError());
    EZ_HIP(hipEventRecord(e1, st));
    long long got[4] = {0, 0, 0, 0};
    EZ_HIP(hipMemcpyAsync(got, p->stats, 32, hipMemcpyDeviceToHost, st));
    EZ_HIP(hipStreamSynchronize(st));
    if (got[2]) {
        t_wit_error = "witness: " + std::to_string(got[2]) + " lookup inputs beyond 62 bits: the columns are not those of a replay that passed";
        return EZKL_ERR_INVALID;
    }
    out_min_max[0] = got[0];
    out_min_max[1] = got[1];
    return EZKL_OK;
}

int ezkl_hip_witness_outputs_dev(ezkl_wplan_t plan, void* const* advice_cols_dev, void* outputs_host, void* stream) {
    if (!plan || !advice_cols_dev) return EZKL_ERR_INVALID;
    t_wit_error.clear();
    DevPlan* p = reinterpret_cast<DevPlan*>(plan);
    const Plan& h = p->host;
    auto refuse = [&](const std::string& why) { t_wit_error = "witness: " + why; return EZKL_ERR_INVALID; };
    if (!h.outputs.empty() && !outputs_host) return EZKL_ERR_INVALID;
    // the cells are read where a finished phase left them: phase 0 must have run to its end on exactly these columns, and no output
    // may sit in a column that a phase not yet finished zero-fills and writes
    if (p->done_phase < 0) return refuse("the outputs before phase 0 has run to its end");
    WitCols cols;
    for (uint32_t j = 0; j < MAX_ADVICE; j++) cols.p[j] = nullptr;
    for (uint32_t j = 0; j < h.n_advice; j++) {
        if (!advice_cols_dev[j]) return EZKL_ERR_INVALID;
        if (advice_cols_dev[j] != p->done_cols[j]) return refuse("the outputs on other columns than the ones phase 0 ran on");
        cols.p[j] = static_cast<fe_t*>(advice_cols_dev[j]);
    }
    for (const uint32_t cell : h.outputs)                          // (cell < n_advice * 2^k: checked on upload)
        if ((int)h.col_phase[cell >> h.k] > p->done_phase)
            return refuse("an output cell belongs to phase " + std::to_string(h.col_phase[cell >> h.k]) + ", which has not run to its end");
    if (h.outputs.empty()) return EZKL_OK;
    EZ_CTX(c);
    if (c != p->ctx) return EZKL_ERR_INVALID;
    hipStream_t st = pick_stream(c, stream);
    hipEvent_t e0, e1;
    int rc = ev_pair(c, "witness_outputs", &e0, &e1);
    if (rc) return rc;
    EZ_HIP(hipEventRecord(e0, st));
    hipLaunchKernelGGL(wit_gather_kernel, dim3(cdiv(h.outputs.size(), 64)), dim3(64), 0, st, cols, h.k, p->outputs, (uint32_t)h.outputs.size(), p->outs);
    EZ_HIP(hipGetLastError());
    EZ_HIP(hipEventRecord(e1, st));
    EZ_HIP(hipMemcpyAsync(outputs_host, p->outs, h.outputs.size() * 32, hipMemcpyDeviceToHost, st));
    EZ_HIP(hipStreamSynchronize(st));
    return EZKL_OK;
}

int ezkl_hip_witness_tile_dev(void* const* advice_cols_dev, uint32_t n_advice, uint32_t k, uint32_t unit_rows, uint32_t tiles, const uint32_t* dst_cols,
                              const uint32_t* src_cols, uint32_t n_pairs, void* stream) {
    if (!advice_cols_dev || n_advice == 0 || n_advice > MAX_ADVICE || k < 1 || k > 28 || (n_pairs && (!dst_cols || !src_cols))) return EZKL_ERR_INVALID;
    if (unit_rows == 0 || tiles == 0 || (uint64_t)unit_rows * tiles > ((uint64_t)1 << k)) return EZKL_ERR_INVALID;
    bool is_dst[MAX_ADVICE] = {false}, is_src_of_other[MAX_ADVICE] = {false};
    for (uint32_t i = 0; i < n_pairs; i++) {
        const uint32_t d = dst_cols[i], s = src_cols[i];
        if (d >= n_advice || s >= n_advice || !advice_cols_dev[d] || !advice_cols_dev[s]) return EZKL_ERR_INVALID;
        if (is_dst[d]) return EZKL_ERR_INVALID;                      // a column appears twice as dst
        is_dst[d] = true;
        if (d != s) is_src_of_other[s] = true;
    }
    WitTile t;
    for (uint32_t i = 0; i < n_pairs; i++) {
        const uint32_t d = dst_cols[i], s = src_cols[i];
        if (d != s && is_src_of_other[d]) return EZKL_ERR_INVALID;   // its rows [0, U) would be written while another pair reads them
        for (uint32_t j = 0; j < n_pairs; j++)                       // two columns on one buffer: the same hazards under other names
            for (const uint32_t o : {dst_cols[j], src_cols[j]})
                if ((o != d && advice_cols_dev[o] == advice_cols_dev[d]) || (o != s && advice_cols_dev[o] == advice_cols_dev[s])) return EZKL_ERR_INVALID;
        t.dst[i] = static_cast<fe_t*>(advice_cols_dev[d]);
        t.src[i] = static_cast<const fe_t*>(advice_cols_dev[s]);
    }
    if (n_pairs == 0) return EZKL_OK;
    EZ_CTX(c);
    hipStream_t st = pick_stream(c, stream);
    hipEvent_t e0, e1;
    int rc = ev_pair(c, "witness_tile", &e0, &e1);
    if (rc) return rc;
    const uint32_t rows = unit_rows * tiles;
    EZ_HIP(hipEventRecord(e0, st));
    hipLaunchKernelGGL(wit_tile_kernel, dim3(cdiv(rows, 256), n_pairs), dim3(256), 0, st, t, unit_rows, rows);
    EZ_HIP(hipGetLastError());
    EZ_HIP(hipEventRecord(e1, st));
    return EZKL_OK;
}

int ezkl_hip_witness_run_dev(ezkl_wplan_t plan, const int64_t* inputs_host, size_t n_inputs, void* const* advice_cols_dev, void* outputs_host,
                             uint64_t status[4], void* stream) {
    if (!plan || !advice_cols_dev || !status || (n_inputs && !inputs_host)) return EZKL_ERR_INVALID;
    const Plan& h = reinterpret_cast<DevPlan*>(plan)->host;
    if (h.n_phases > 1) {
        memset(status, 0, 4 * sizeof(uint64_t));
        t_wit_error = "witness: a plan with " + std::to_string(h.n_phases) + " phases runs phase by phase: ezkl_hip_witness_run_phase_dev";
        return EZKL_ERR_INVALID;
    }
    if (n_inputs != h.n_inputs || (!h.outputs.empty() && !outputs_host)) return EZKL_ERR_INVALID;
    return ezkl_hip_witness_run_phase_dev(plan, 0, inputs_host, n_inputs, nullptr, 0, advice_cols_dev, outputs_host, status, stream);
}

}  // extern "C"
