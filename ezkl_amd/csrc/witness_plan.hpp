// witness_plan.hpp -- the witness-plan blob (ezkl_amd/witness_plan.py writes it) parsed and validated on the host.  Plain C++, no device
// code: libezkl_hip.so runs it before a plan reaches the device (ezkl_hip_witness_plan_upload), libezkl_prover.so exposes it as
// ezkl_prover_witness_plan_check so that the sanitizer build (tools/asan_run.sh) covers it.  witness_plan.validate is its Python mirror.
//
// Layout (little-endian): 20 x u32 header -- magic "EZWP", version, k, n_advice, n_records, n_inputs, n_params, n_consts, n_outputs,
// n_cells, n_words, n_ops, n_tables, n_table_values, n_challenges, n_phases (0 reads as 1), 4 reserved -- and the 32-byte parameter hash;
// then n_params x int64, n_consts x
// 32 bytes (canonical Fr), n_records x {kind, count, p0, p1, dst, a, b, phase}, n_outputs x u32 cells, n_words x u32 pool, n_tables x
// {lo (int32), n, col_size, offset} and n_table_values x int64: the static lookup tables, f(lo + i) as signed integers (both sections
// are empty in a plan without lookups: the two header words were reserved zeros).  Cells are numbered column * 2^k + row.
// A TABLE / TBLIDX record: a = source cell, p0 = table index; with s the signed value of the cell, values[offset + (s - lo)] as a field
// element / (s - lo) // col_size.  s outside [lo, lo + n - 1] is a run-time failure of the lane, as a value beyond its decomposition is.
// PHASES (second-phase advice: the Freivalds einsum).  Header words 14 / 15 and the eighth word of a record were reserved zeros, so every
// one-phase blob keeps its bytes.  A record is replayed by the run of its phase; phases are non-decreasing along the list and below
// n_phases; a column belongs to the phase of the records that write it (two phases: refused; no record: phase 0); INPUT and MATMUL records
// belong to phase 0, with which the inputs are uploaded.
// A MATMUL record: count = m * n, p0 = kd, p1 = n; dst = m * n cells row-major, a = m * kd and b = kd * n INPUT indices;
// dst[i * n + j] = sum_t in[a[i * kd + t]] * in[b[t * n + j]] over the integers, then integer_rep_to_felt.  Every operand must satisfy
// |v| < 2^31 (kd * 2^62 < 2^127: two 64-bit words hold the sum); one outside is a run-time failure of the lane, element = its place in a, or
// m * kd + its place in b.
// An RLC record: count scans of p1 steps with challenge p0 (< n_challenges), step-major and dense (no 0xffffffff entries): out[0] = c * v[0],
// out[t] = out[t - 1] * c + c * v[t], v[t] = cell a[t * count + d], out[t] -> cell dst[t * count + d].
// A DIVC record (the rebase division of an MLP layer, layouts.rs:219-267 `div`): a = source cell, p0 = d >= 1 (zero: refused); with s the
// signed value of the cell, sgn(s) * ((|s| + d / 2) / d) -- s / d rounded half away from zero.  |s| >= 2^52 is a run-time failure of the lane.
// Kind 16 is unassigned (refused as an unknown kind); SUMACC, PRODACC, GATHER and CLAMP are 17 .. 20.
// A SUMACC / PRODACC record (BaseRegion._accumulate, layouts.rs:2472-2621 `sum` / `prod`): count scans of p1 steps with p0 operands each,
// step-major as DOT is; step s of scan d folds the cells a[(s * p0 + j) * count + d], j < p0 (0xffffffff: no operand -- the duplicated row
// at the top of a new column), into the running value (0 at the start of a sum, 1 of a product) and writes it to dst[s * count + d]
// (0xffffffff: the scan has no such step: a ragged record).  b is unused and zero.  p0 or p1 zero, or an index array past the pool: "bad
// scan shape".
// A GATHER record: a = the cell holding the index, p0 = the pool offset of the table's cell list, p1 = its length n >= 1 ("empty gather
// table", "gather table runs past the pool"); with s the signed value of the index cell the destination gets the value of cell
// pool[p0 + s].  Every cell of the list is one a lane can read: in range and written by an earlier record.  s < 0, s >= n or |s| >= 2^62
// is a run-time failure of the lane ("gather index outside the table"), tested before pool[p0 + s] is read.
// A CLAMP record: a = source cell, p0 = lo, p1 = hi (int32, lo <= hi, else "bad clamp bounds"): min(max(s, lo), hi); a value beyond 62 bits
// clamps by its sign.  It never fails.
// A SORT (21) / ARGSORT (22) record (layouts.rs:1158-1275 `_sort_ascending`, the witness of its sorted tensor and of the claimed indices of
// `shuffles`): count destination cells dst[e] in segments of p0 = n elements (n >= 1, count % n == 0, count <= 2^28, else "bad sort shape"),
// p1 = mode (0 or 1, else "bad sort shape"), a = the source cells, segment-major and dense, b unused and zero.  The order of a segment is
// by (signed value, position), the position ascending among equal values for mode 0 and descending for mode 1: a total order.  SORT:
// dst[s * n + i] gets the i-th smallest signed value of the cells a[s * n .. + n) as integer_rep_to_felt maps it; ARGSORT: the position, in
// [0, n), of that element in its segment.  A source with |s| >= 2^62 is a run-time failure of the lane ("sort key beyond 62 bits"), element
// = its place in a; its segment writes none of its cells.  SORT_TILE is the number of keys one workgroup of csrc/witness.hip sorts in LDS.
// Kind 23 (N_KINDS, the end of KIND_NAMES) is unassigned as 16 is; RECIP and ISQRT are 24 and 25, KINDS_END follows them, `kind_name`
// names every kind.
// A RECIP record (the claimed reciprocal of `recip`, layouts.rs:300-385): a = source cell, b = the index of `zero_inverse` in the constants
// section (a scalar word, not a pool offset: past the constants is "zero-inverse index past the constants"), S = p0 | p1 << 32 = input
// scale * output scale, 1 <= S < 2^62 (else "reciprocal scale outside [1, 2^62)").  With x the signed value of the cell: x = 0 -> the
// constant; x > 0 -> ceil((2S - x) / (2x)) = (2S + x - 1) / (2x); x < 0 -> -((2S + |x|) / (2|x|)) -- the one value the gates of
// `optimum_convex_function` accept, the smallest integer minimiser of |y * x - S|.  |x| >= 2^62 is a run-time failure of the lane
// ("reciprocal operand beyond 62 bits").
// An ISQRT record (the claimed root of `sqrt`, layouts.rs:408-459): a = source cell, b = 0, p0 = input scale >= 1 ("zero square-root
// scale"), p1 = 0 ("a square-root record with a second parameter").  With T = x * p0: T <= 0 -> 0; else r = floor(sqrt(T)), r + (T - r * r > r),
// the integer nearest to sqrt(T).  |x| >= 2^62 or T >= 2^62 is a run-time failure of the lane ("square-root operand outside the exact range").
// Kind 26 (KINDS_END) is unassigned as 16 and 23 are; ARGEXT is 27 and KINDS_LIMIT follows it.
// An ARGEXT record (the claimed index of `argmax` / `argmin`, layouts.rs:5225-5293, which the prover states BEFORE the sort that checks it):
// count = the number of segments = the number of destination cells dst[s], p0 = n >= 1 the segment length, p1 = mode (0: argmax, 1: argmin),
// a = count * n source cells, segment-major and dense, b unused and zero.  p0 == 0, p1 > 1, count * p0 > 2^28 or an array past the pool:
// "bad arg-extremum shape".  dst[s] gets the SMALLEST position j in [0, n) whose signed value is the greatest (mode 0) or the least (mode 1)
// of the cells a[s * n .. + n): the reference's max_by_key((value, -idx)) / min_by_key((value, idx)), the one claim the gates accept.  A
// source with |s| >= 2^62 is a run-time failure of the lane ("arg-extremum key beyond 62 bits"), element = its place in a; its segment's
// cell is not written.  ARGEXT_CHUNK is the number of sources one workgroup of csrc/witness.hip reduces.
// Kind 28 (KINDS_LIMIT) is unassigned as 16, 23 and 26 are; SCATTER, COMPLEMENT and ONEHOT are 29 .. 31 and KINDS_TOP follows them.
// A SCATTER record (the claimed output of `scatter_elements`, layouts.rs:2313-2379, which the prover states BEFORE the gathers that check it):
// ONE tensor -- count = n destination cells dst[i], a = the n base cells, p0 = m >= 1 elements, p1 = the multiplier of the scattered dimension
// >= 1, b = the pool offset of 1 + 3m words: the extent of that dimension, m index cells, m source cells, m constant offsets (plain words).
// With s_j the signed value of index cell j its target is t_j = s_j * p1 + off_j; dst[i] gets the value of source cell j for the GREATEST j
// with t_j == i (tensor::ops::scatter: the later element wins), else the value of base cell i.  p0, p1 or the extent zero, count > 2^28, an
// array past the pool or an offset with off_j + (extent - 1) * p1 >= count: "bad scatter shape" -- so every target of an index inside
// [0, extent) is a destination.  s_j < 0, s_j >= extent or |s_j| >= 2^62 is a run-time failure of the lane ("scatter index outside the
// tensor"), element = j, every such j counted; the record then writes none of its cells.  SCATTER_TILE is the number of destinations one
// workgroup of csrc/witness.hip resolves in LDS.
// A COMPLEMENT record (the claimed output of `get_missing_set_elements` over the positions, layouts.rs:2213-2286): p0 = n, the set {0 .. n - 1},
// p1 = m <= n source cells at a, count = n - m destination cells (zero is legal: the record writes nothing), b unused and zero.  dst[i] gets
// the i-th smallest v in [0, n) that is the signed value of no source cell; a source outside [0, n) or beyond 62 bits removes nothing.  It
// never fails.  p1 > p0, count != p0 - p1, p0 > 2^28 or an array past the pool: "bad complement shape".
// A ONEHOT record (the claimed vector of `one_hot`, layouts.rs:1398-1442), element-wise: a = the index cell of element e, b = the pool
// offset of the per-element positions (plain words), p0 = num_classes >= 1 ("zero one-hot classes"), p1 = 0: 1 if the signed value equals
// the position, else 0.  s < 0, s >= p0 or |s| >= 2^62 is a run-time failure of the lane ("one-hot index outside the classes").
#pragma once
#include <stdint.h>
#include <algorithm>
#include <string.h>
#include <string>
#include <vector>

namespace ezkl {
namespace wplan {

constexpr uint32_t MAGIC = 0x50575A45u, VERSION = 1, NONE = 0xFFFFFFFFu, MAX_ADVICE = 64, MAX_PHASES = 3, MAX_CHALLENGES = 64, SORT_TILE = 2048,
                   MAX_SORT_COUNT = 1u << 28, ARGEXT_CHUNK = 4096, SCATTER_TILE = 4096;
enum Kind : uint32_t { COPY, CONST, INPUT, PARAM, ADD, SUB, MUL, HINT, RCIDX, INVZ, DOT, TABLE, TBLIDX, MATMUL, RLC, DIVC, UNASSIGNED, SUMACC, PRODACC, GATHER, CLAMP, SORT, ARGSORT, N_KINDS,     // 16 names nothing: refused as unknown
                       RECIP = 24, ISQRT = 25, KINDS_END,                         // N_KINDS ends KIND_NAMES and, as a kind (23), names nothing either
                       ARGEXT = 27, KINDS_LIMIT,                                   // KINDS_END (26) names nothing either; KINDS_LIMIT (28) was the first kind past them all and names nothing
                       SCATTER = 29, COMPLEMENT = 30, ONEHOT = 31, KINDS_TOP };    // KINDS_TOP is the first kind past them all
static const char* const KIND_NAMES[N_KINDS] = {"copy", "const", "input", "param", "add", "sub", "mult", "decompose", "range_check", "equals_zero", "dot",
                                                "nonlinearity", "nonlinearity_index", "matmul", "rlc", "div", "?", "sum", "prod", "gather", "clamp", "sort", "argsort"};
// the name a message gives a kind: KIND_NAMES up to ARGSORT, the later kinds by hand, "?" for a kind that names nothing
inline const char* kind_name(uint32_t kind) { return kind < N_KINDS ? KIND_NAMES[kind] : kind == RECIP ? "recip" : kind == ISQRT ? "sqrt" : kind == ARGEXT ? "argext" : kind == SCATTER ? "scatter" : kind == COMPLEMENT ? "complement" : kind == ONEHOT ? "one_hot" : "?"; }
struct Rec {
    uint32_t kind, count, p0, p1, dst, a, b, phase;
};
struct Table {
    int32_t lo;
    uint32_t n, col_size, off;
};
struct Plan {
    uint32_t k = 0, n_advice = 0, n_inputs = 0, n_cells = 0, n_ops = 0, n_challenges = 0, n_phases = 1;
    uint8_t col_phase[MAX_ADVICE] = {0};       // the phase each column belongs to (a column no record writes: 0)
    uint8_t param_hash[32] = {0};
    std::vector<int64_t> params;
    std::vector<uint8_t> consts;       // 32 bytes each, canonical
    std::vector<Rec> recs;
    std::vector<uint32_t> outputs, pool;
    std::vector<Table> tables;
    std::vector<int64_t> table_values;
};
// BN254 Fr modulus, little-endian bytes (a constant, and a challenge, must be canonical)
static const uint8_t FR_MOD_LE[32] = {0x01, 0x00, 0x00, 0xf0, 0x93, 0xf5, 0xe1, 0x43, 0x91, 0x70, 0xb9, 0x79, 0x48, 0xe8, 0x33, 0x28,
                                      0x5d, 0x58, 0x81, 0x81, 0xb6, 0x45, 0x50, 0xb8, 0x29, 0xa0, 0x31, 0xe1, 0x72, 0x4e, 0x64, 0x30};

// the set of cells written so far.  Its memory is bounded by the BLOB, not by the geometry two header words claim: one bit per cell
// when that is no more than the pool itself (a laid-out circuit: most cells are written), otherwise one bit per distinct pool word
// (every cell a record can name is a pool word), found by binary search.
class Written {
    std::vector<uint64_t> w;
    std::vector<uint32_t> keys;        // sparse form: the distinct pool words, sorted
    bool dense;
    uint64_t at(uint32_t cell) const { return dense ? cell : (uint64_t)(std::lower_bound(keys.begin(), keys.end(), cell) - keys.begin()); }
public:
    Written(uint64_t cells, const std::vector<uint32_t>& pool) : dense(cells <= 32 * (uint64_t)pool.size() + ((uint64_t)1 << 19)) {
        if (!dense) {
            keys = pool;
            std::sort(keys.begin(), keys.end());
            keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
        }
        w.assign(((dense ? cells : keys.size()) + 63) / 64, 0);
    }
    bool get(uint32_t cell) const {
        const uint64_t i = at(cell);
        if (!dense && (i >= keys.size() || keys[i] != cell)) return false;     // not a pool word (an output cell can be anything)
        return (w[i >> 6] >> (i & 63)) & 1;
    }
    void set(uint32_t cell) { const uint64_t i = at(cell); w[i >> 6] |= (uint64_t)1 << (i & 63); }
};

inline bool canonical(const uint8_t* c) {                 // below the modulus, compared from the top byte down
    int j = 31;
    while (j >= 0 && c[j] == FR_MOD_LE[j]) j--;
    return j >= 0 && c[j] < FR_MOD_LE[j];
}

// parse + validate; false with `why` set when the blob is refused.  Everything the kernels index with is checked here: every cell
// index < n_advice * 2^k, every table index in range, every pool span inside the pool, each cell written at most once and read only
// after an EARLIER record has written it; the phases are non-decreasing and every column is written in one phase only.
inline bool parse(const void* blob, size_t len, Plan& out, std::string& why) {
    auto fail = [&](const std::string& s) { why = "witness plan: " + s; return false; };
    auto at_rec = [&](size_t ri, uint32_t kind, const char* s) { return fail("record " + std::to_string(ri) + " (" + kind_name(kind) + "): " + s); };
    const uint8_t* p = static_cast<const uint8_t*>(blob);
    uint32_t h[20];
    if (!blob || len < sizeof h + 32) return fail("shorter than its header");
    memcpy(h, p, sizeof h);
    if (h[0] != MAGIC) return fail("bad magic");
    if (h[1] != VERSION) return fail("version " + std::to_string(h[1]) + ", this build reads " + std::to_string(VERSION));
    const uint32_t k = h[2], n_adv = h[3], n_rec = h[4], n_in = h[5], n_par = h[6], n_con = h[7], n_out = h[8], n_cells = h[9], n_words = h[10], n_tab = h[12], n_val = h[13];
    if (k < 1 || k > 28 || n_adv == 0 || n_adv > MAX_ADVICE || ((uint64_t)n_adv << k) > ((uint64_t)1 << 32)) return fail("bad geometry");
    const uint32_t n_chal = h[14], n_phases = h[15] ? h[15] : 1;
    if (n_phases > MAX_PHASES || n_chal > MAX_CHALLENGES) return fail("bad phase or challenge count");
    const uint64_t want = (uint64_t)sizeof h + 32 + 8ull * n_par + 32ull * n_con + 32ull * n_rec + 4ull * n_out + 4ull * n_words + 16ull * n_tab + 8ull * n_val;
    if (want != len) return fail(std::to_string(len) + " bytes, its header says " + std::to_string(want));
    out.k = k; out.n_advice = n_adv; out.n_inputs = n_in; out.n_cells = n_cells; out.n_ops = h[11]; out.n_challenges = n_chal; out.n_phases = n_phases;
    p += sizeof h;
    memcpy(out.param_hash, p, 32); p += 32;
    out.params.resize(n_par);   if (n_par) memcpy(out.params.data(), p, 8ull * n_par);   p += 8ull * n_par;
    out.consts.resize(32ull * n_con); if (n_con) memcpy(out.consts.data(), p, 32ull * n_con); p += 32ull * n_con;
    out.recs.resize(n_rec);     if (n_rec) memcpy(out.recs.data(), p, 32ull * n_rec);    p += 32ull * n_rec;
    out.outputs.resize(n_out);  if (n_out) memcpy(out.outputs.data(), p, 4ull * n_out);  p += 4ull * n_out;
    out.pool.resize(n_words);   if (n_words) memcpy(out.pool.data(), p, 4ull * n_words);  p += 4ull * n_words;
    out.tables.resize(n_tab);   if (n_tab) memcpy(out.tables.data(), p, 16ull * n_tab);   p += 16ull * n_tab;
    out.table_values.resize(n_val); if (n_val) memcpy(out.table_values.data(), p, 8ull * n_val);
    for (uint32_t i = 0; i < n_con; i++)
        if (!canonical(out.consts.data() + 32ull * i)) return fail("a constant is not a canonical field element");
    for (size_t ti = 0; ti < out.tables.size(); ti++) {
        const Table& t = out.tables[ti];
        if (t.n < 1 || t.col_size < 1 || (int64_t)t.lo + t.n - 1 > 0x7fffffffll) return fail("table " + std::to_string(ti) + ": bad lookup table shape");
        if (t.off > n_val || t.n > n_val - t.off) return fail("table " + std::to_string(ti) + ": runs past the table values");
    }
    const uint64_t cells = (uint64_t)n_adv << k;
    if (n_cells > n_words) return fail("more cells than index words");
    Written written(cells, out.pool);
    uint64_t total = 0;
    const std::vector<uint32_t>& P = out.pool;
    auto span_ok = [&](uint32_t off, uint64_t n) { return off <= P.size() && n <= P.size() - off; };
    int col_phase[MAX_ADVICE];
    for (uint32_t c = 0; c < MAX_ADVICE; c++) col_phase[c] = -1;
    uint32_t last_phase = 0;
    for (size_t ri = 0; ri < out.recs.size(); ri++) {
        const Rec& r = out.recs[ri];
        if (r.kind >= KINDS_TOP || r.kind == KINDS_LIMIT || r.kind == KINDS_END || r.kind == N_KINDS || r.kind == UNASSIGNED) return at_rec(ri, r.kind, "unknown kind");
        if (r.count == 0 && r.kind != COMPLEMENT) return at_rec(ri, r.kind, "empty");     // (nothing missing: a complement that writes no cell)
        if (r.phase >= n_phases) return at_rec(ri, r.kind, "phase out of range");
        if (r.phase < last_phase) return at_rec(ri, r.kind, "phases decrease");
        last_phase = r.phase;
        if ((r.kind == INPUT || r.kind == MATMUL) && r.phase != 0) return at_rec(ri, r.kind, "input and matmul records belong to phase 0");
        uint64_t n_dst = r.count, n_a = r.count, n_b = 0;
        bool a_cells = false, b_cells = false;
        uint32_t a_lim = 0;
        switch (r.kind) {
        case COPY: case INVZ: a_cells = true; break;
        case ADD: case SUB: case MUL: a_cells = b_cells = true; n_b = r.count; break;
        case CONST: a_lim = n_con; break;
        case INPUT: a_lim = n_in; break;
        case PARAM: a_lim = n_par; break;
        case HINT: {
            a_cells = true; n_b = r.count;
            uint64_t bound = 1;
            if (r.p0 < 2 || r.p1 == 0) return at_rec(ri, r.kind, "bad decomposition");
            for (uint32_t t = 0; t < r.p1; t++) {
                if (bound > (((uint64_t)1 << 62) - 1) / r.p0) return at_rec(ri, r.kind, "bad decomposition");     // base^legs < 2^62, without overflow
                bound *= r.p0;
            }
            break;
        }
        case RCIDX: a_cells = true; if (r.p1 == 0) return at_rec(ri, r.kind, "zero table column size"); break;
        case DIVC: a_cells = true; if (r.p0 == 0) return at_rec(ri, r.kind, "zero divisor"); break;
        case TABLE: case TBLIDX: a_cells = true; if (r.p0 >= n_tab) return at_rec(ri, r.kind, "lookup table index out of range"); break;
        case MATMUL: {                                   // p0 = kd, p1 = n, count = m * n: a = m * kd, b = kd * n input indices
            if (r.p0 == 0 || r.p1 == 0 || r.count % r.p1 != 0) return at_rec(ri, r.kind, "bad matmul shape");
            n_a = (uint64_t)(r.count / r.p1) * r.p0; n_b = (uint64_t)r.p0 * r.p1; a_lim = n_in;
            if (!span_ok(r.dst, n_dst) || !span_ok(r.a, n_a) || !span_ok(r.b, n_b)) return at_rec(ri, r.kind, "bad matmul shape");
            break;
        }
        case RLC:                                        // p0 = challenge, p1 = steps, count = scans
            if (r.p0 >= n_chal) return at_rec(ri, r.kind, "challenge index out of range");
            if (r.p1 == 0 || (uint64_t)r.count * r.p1 > P.size()) return at_rec(ri, r.kind, "bad rlc shape");
            n_dst = n_a = (uint64_t)r.count * r.p1; a_cells = true;
            break;
        case SUMACC: case PRODACC:                       // p0 = operands per step, p1 = steps, count = scans
            if (r.p0 == 0 || r.p1 == 0 || !span_ok(r.dst, (uint64_t)r.count * r.p1) || !span_ok(r.a, (uint64_t)r.count * r.p1 * r.p0)) return at_rec(ri, r.kind, "bad scan shape");
            n_dst = (uint64_t)r.count * r.p1; n_a = n_dst * r.p0; a_cells = true;
            break;
        case GATHER: {                                   // p0 = pool offset of the table's cell list, p1 = its length
            a_cells = true;
            if (r.p1 == 0) return at_rec(ri, r.kind, "empty gather table");
            if (!span_ok(r.p0, r.p1)) return at_rec(ri, r.kind, "gather table runs past the pool");
            for (uint32_t i = 0; i < r.p1; i++) {        // every cell of the table is one a lane can read
                const uint32_t x = P[r.p0 + i];
                if (x >= cells) return at_rec(ri, r.kind, "cell index out of range");
                if (!written.get(x)) return at_rec(ri, r.kind, "a cell is read before an earlier record has written it");
            }
            break;
        }
        case CLAMP: a_cells = true; if ((int32_t)r.p0 > (int32_t)r.p1) return at_rec(ri, r.kind, "bad clamp bounds"); break;
        case SORT: case ARGSORT:                         // p0 = segment length, p1 = mode, count = segments * p0
            if (r.p0 == 0 || r.count % r.p0 != 0 || r.p1 > 1 || r.count > MAX_SORT_COUNT) return at_rec(ri, r.kind, "bad sort shape");
            a_cells = true;
            break;
        case RECIP: {                                    // S = p0 | p1 << 32, b = the constant a zero input takes
            a_cells = true;
            const uint64_t S = (uint64_t)r.p0 | ((uint64_t)r.p1 << 32);
            if (S == 0 || S >= ((uint64_t)1 << 62)) return at_rec(ri, r.kind, "reciprocal scale outside [1, 2^62)");
            if (r.b >= n_con) return at_rec(ri, r.kind, "zero-inverse index past the constants");
            break;
        }
        case ISQRT:
            a_cells = true;
            if (r.p0 == 0) return at_rec(ri, r.kind, "zero square-root scale");
            if (r.p1 != 0) return at_rec(ri, r.kind, "a square-root record with a second parameter");
            break;
        case ARGEXT:                                     // p0 = segment length, p1 = mode, count = segments = destination cells
            if (r.p0 == 0 || r.p1 > 1 || (uint64_t)r.count * r.p0 > MAX_SORT_COUNT || !span_ok(r.dst, r.count) || !span_ok(r.a, (uint64_t)r.count * r.p0))
                return at_rec(ri, r.kind, "bad arg-extremum shape");
            n_a = (uint64_t)r.count * r.p0; a_cells = true;
            break;
        case SCATTER: {                                  // p0 = elements, p1 = multiplier, b: extent, index cells, source cells, offsets
            if (r.p0 == 0 || r.p1 == 0 || r.count > MAX_SORT_COUNT || !span_ok(r.dst, r.count) || !span_ok(r.a, r.count) || !span_ok(r.b, 1 + 3ull * r.p0))
                return at_rec(ri, r.kind, "bad scatter shape");
            const uint32_t extent = P[r.b];
            if (extent == 0) return at_rec(ri, r.kind, "bad scatter shape");
            for (uint32_t j = 0; j < r.p0; j++)          // every target of an index inside [0, extent) is a destination: no overflow, both factors are 32-bit
                if ((uint64_t)P[r.b + 1 + 2ull * r.p0 + j] + (uint64_t)(extent - 1) * r.p1 >= r.count) return at_rec(ri, r.kind, "bad scatter shape");
            for (uint64_t j = 0; j < 2ull * r.p0; j++) {   // the index and source cells: ones a lane can read
                const uint32_t x = P[r.b + 1 + j];
                if (x >= cells) return at_rec(ri, r.kind, "cell index out of range");
                if (!written.get(x)) return at_rec(ri, r.kind, "a cell is read before an earlier record has written it");
            }
            a_cells = true;
            break;
        }
        case COMPLEMENT:                                 // p0 = n, p1 = sources, count = n - sources
            if (r.p1 > r.p0 || r.count != r.p0 - r.p1 || r.p0 > MAX_SORT_COUNT || !span_ok(r.dst, r.count) || !span_ok(r.a, r.p1)) return at_rec(ri, r.kind, "bad complement shape");
            n_a = r.p1; a_cells = true;
            break;
        case ONEHOT: a_cells = true; n_b = r.count; if (r.p0 == 0) return at_rec(ri, r.kind, "zero one-hot classes"); break;
        case DOT:
            if (r.p0 == 0 || r.p1 == 0 || (uint64_t)r.count * r.p1 > P.size() || (uint64_t)r.count * r.p1 * r.p0 > P.size()) return at_rec(ri, r.kind, "bad dot shape");
            n_dst = (uint64_t)r.count * r.p1; n_a = n_b = n_dst * r.p0; a_cells = b_cells = true;
            break;
        }
        if (!span_ok(r.dst, n_dst) || !span_ok(r.a, n_a) || (r.kind != RECIP && r.kind != SCATTER && !span_ok(r.b, n_b)))     // (RECIP: b is no pool offset; SCATTER: checked above)
            return at_rec(ri, r.kind, "an index array runs past the pool");
        const bool sparse = r.kind == DOT || r.kind == SUMACC || r.kind == PRODACC;     // 0xffffffff = no entry
        for (uint64_t i = 0; i < n_a; i++) {
            const uint32_t x = P[r.a + i];
            if (sparse && x == NONE) {
                if (r.kind == DOT && P[r.b + i] != NONE) return at_rec(ri, r.kind, "a product with one operand");
                continue;
            }
            if (a_cells) {
                if (x >= cells) return at_rec(ri, r.kind, "cell index out of range");
                if (!written.get(x)) return at_rec(ri, r.kind, "a cell is read before an earlier record has written it");
            } else if (x >= a_lim) return at_rec(ri, r.kind, "table index out of range");
        }
        for (uint64_t i = 0; i < n_b; i++) {
            const uint32_t x = P[r.b + i];
            if (r.kind == HINT) {
                if (x != NONE && x >= r.p1) return at_rec(ri, r.kind, "bad decomposition");
                continue;
            }
            if (r.kind == ONEHOT) continue;              // positions: plain words
            if (sparse && x == NONE) {
                if (P[r.a + i] != NONE) return at_rec(ri, r.kind, "a product with one operand");
                continue;
            }
            if (r.kind == MATMUL) {
                if (x >= a_lim) return at_rec(ri, r.kind, "table index out of range");
                continue;
            }
            if (b_cells) {
                if (x >= cells) return at_rec(ri, r.kind, "cell index out of range");
                if (!written.get(x)) return at_rec(ri, r.kind, "a cell is read before an earlier record has written it");
            }
        }
        // destinations after every source of the record: a record never reads what it writes
        for (uint64_t i = 0; i < n_dst; i++) {
            const uint32_t x = P[r.dst + i];
            if (sparse && x == NONE) continue;
            if (x >= cells) return at_rec(ri, r.kind, "cell index out of range");
        }
        for (uint64_t i = 0; i < n_dst; i++) {
            const uint32_t x = P[r.dst + i];
            if (sparse && x == NONE) continue;
            if (written.get(x)) return at_rec(ri, r.kind, "a cell is written twice");
            written.set(x);
            total++;
        }
        for (uint64_t i = 0; i < n_dst; i++) {
            const uint32_t x = P[r.dst + i];
            if (sparse && x == NONE) continue;
            int& cp = col_phase[x >> k];
            if (cp >= 0 && cp != (int)r.phase) return at_rec(ri, r.kind, "a column is written in two phases");
            cp = (int)r.phase;
        }
    }
    if (total != n_cells) return fail(std::to_string(total) + " cells written, its header says " + std::to_string(n_cells));
    for (uint32_t c : out.outputs)
        if (c >= cells || !written.get(c)) return fail("an output cell is never written");
    for (uint32_t c = 0; c < n_adv; c++) out.col_phase[c] = col_phase[c] < 0 ? 0 : (uint8_t)col_phase[c];
    return true;
}

}  // namespace wplan
}  // namespace ezkl
