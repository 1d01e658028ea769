// witness_plan.hpp -- the witness-plan blob (ezkl_amd/witness_plan.py writes it) parsed and validated on the host.  Plain C++, no device
// code: libezkl_hip.so runs it before a plan reaches the device (ezkl_hip_witness_plan_upload), libezkl_prover.so exposes it as
// ezkl_prover_witness_plan_check so that the sanitizer build (tools/asan_run.sh) covers it.  witness_plan.validate is its Python mirror.
//
// Layout (little-endian): 20 x u32 header -- magic "EZWP", version, k, n_advice, n_records, n_inputs, n_params, n_consts, n_outputs,
// n_cells, n_words, n_ops, n_tables, n_table_values, n_challenges, n_phases (0 reads as 1), 4 reserved -- and the 32-byte parameter hash;
// then n_params x int64, n_consts x 32 bytes (canonical Fr), n_records x {kind, count, p0, p1, dst, a, b, phase}, n_outputs x u32 cells,
// n_words x u32 pool, n_tables x {lo (int32), n, col_size, offset} and n_table_values x int64: the static lookup tables, f(lo + i) as signed
// integers (both sections are empty in a plan without lookups).  Cells are numbered column * 2^k + row.
//
// What every kind of record means, its parameters and its run-time failure: the module docstring of ezkl_amd/witness_plan.py, kind by kind;
// `run_plan_host` there is the executable form.  KINDS below is the same table as KINDS there (tests/test_witness_plan_table.py).
//
// What `parse` guarantees to the kernels of csrc/witness.hip: every record is of a known kind with the parameters that kind allows; every
// span a record names lies inside the pool; every word a lane uses as a cell is below n_advice * 2^k, every index below the section it
// points into; a cell is written at most once and read only after an EARLIER record has written it; the phases are non-decreasing, below
// n_phases, and every column is written in one phase only (INPUT and MATMUL records in phase 0, with which the inputs are uploaded).
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
// A DOT record of ONE step (p1 == 1) with p0 >= DOT_WIDE_MIN products -- the claimed product of an einsum -- runs on wit_dot_wide_kernel;
// every other DOT record on wit_dot_kernel.  DOT_WIDE_FILL: the lanes that fill the device (256 compute units x 4 SIMDs x 2 waves of 64).
constexpr uint32_t DOT_WIDE_MIN = 16, DOT_WIDE_FILL = 1u << 17;
// how many lanes of a wave share one dot of the wide kernel: a power of two, at most 64 and at most p0; one when `count` dots alone fill
// the device, more when there are few long dots
inline uint32_t dot_wide_lanes(uint32_t count, uint32_t p0) {
    uint32_t g = 1;
    while (g < 64 && 2 * g <= p0 && (uint64_t)count * g < DOT_WIDE_FILL) g *= 2;
    return g;
}
// kinds 16, 23, 26 and 28 are unassigned and refused; KINDS_TOP is the first kind past them all
enum Kind : uint32_t { COPY, CONST, INPUT, PARAM, ADD, SUB, MUL, HINT, RCIDX, INVZ, DOT, TABLE, TBLIDX, MATMUL, RLC, DIVC, SUMACC = 17, PRODACC, GATHER, CLAMP, SORT, ARGSORT,
                       RECIP = 24, ISQRT, ARGEXT = 27, SCATTER = 29, COMPLEMENT, ONEHOT, KINDS_TOP };
// what the words at a record's a or b are: cells a lane reads, indices below a limit the record's case names (DIGITS: 0xffffffff too, the
// sign), plain words (none of them where the kind does not use the array), or no pool offset at all
enum Role : uint8_t { CELLS, INDICES, DIGITS, WORDS, NOT_POOL };
struct KindInfo {
    const char* name;         // what a message calls the kind; "?": the number names nothing
    const char* failure;      // the words of its run-time failure; nullptr: a lane of this kind never fails
    const char* unit;         // what the count of a run-time failure counts
    bool scan, sparse;        // count * p1 destination words, not count; 0xffffffff in dst, a or b is "no entry"
    Role a, b;
};
static const KindInfo KINDS[KINDS_TOP] = {
    {"copy", nullptr, "cells", false, false, CELLS, WORDS},                                                             //  0
    {"const", nullptr, "cells", false, false, INDICES, WORDS},
    {"input", nullptr, "cells", false, false, INDICES, WORDS},
    {"param", nullptr, "cells", false, false, INDICES, WORDS},
    {"add", nullptr, "cells", false, false, CELLS, CELLS},                                                              //  4
    {"sub", nullptr, "cells", false, false, CELLS, CELLS},
    {"mult", nullptr, "cells", false, false, CELLS, CELLS},
    {"decompose", "value exceeds the decomposition range", "cells", false, false, CELLS, DIGITS},
    {"range_check", "value exceeds the decomposition range", "cells", false, false, CELLS, WORDS},                      //  8
    {"equals_zero", nullptr, "cells", false, false, CELLS, WORDS},
    {"dot", nullptr, "cells", true, true, CELLS, CELLS},
    {"nonlinearity", "lookup input outside the table range", "cells", false, false, CELLS, WORDS},
    {"nonlinearity_index", "lookup input outside the table range", "cells", false, false, CELLS, WORDS},               // 12
    {"matmul", "einsum operand outside the exact-product range", "operand reads", false, false, INDICES, INDICES},
    {"rlc", nullptr, "cells", true, false, CELLS, WORDS},
    {"div", "rebase dividend outside the exact-division range", "cells", false, false, CELLS, WORDS},
    {"?", nullptr, "cells", false, false, WORDS, WORDS},                                                                // 16
    {"sum", nullptr, "cells", true, true, CELLS, WORDS},
    {"prod", nullptr, "cells", true, true, CELLS, WORDS},
    {"gather", "gather index outside the table", "cells", false, false, CELLS, WORDS},
    {"clamp", nullptr, "cells", false, false, CELLS, WORDS},                                                            // 20
    {"sort", "sort key beyond 62 bits", "cells", false, false, CELLS, WORDS},
    {"argsort", "sort key beyond 62 bits", "cells", false, false, CELLS, WORDS},
    {"?", nullptr, "cells", false, false, WORDS, WORDS},
    {"recip", "reciprocal operand beyond 62 bits", "cells", false, false, CELLS, NOT_POOL},                             // 24
    {"sqrt", "square-root operand outside the exact range", "cells", false, false, CELLS, WORDS},
    {"?", nullptr, "cells", false, false, WORDS, WORDS},
    {"argext", "arg-extremum key beyond 62 bits", "cells", false, false, CELLS, WORDS},
    {"?", nullptr, "cells", false, false, WORDS, WORDS},                                                                // 28
    {"scatter", "scatter index outside the tensor", "cells", false, false, CELLS, WORDS},
    {"complement", nullptr, "cells", false, false, CELLS, WORDS},
    {"one_hot", "one-hot index outside the classes", "cells", false, false, CELLS, WORDS},
};
inline bool known(uint32_t kind) { return kind < KINDS_TOP && KINDS[kind].name[0] != '?'; }
inline const char* kind_name(uint32_t kind) { return kind < KINDS_TOP ? KINDS[kind].name : "?"; }     // the name a message gives a kind
// the words a lane's run-time failure is reported with; a kind that has none is reported as a value beyond its decomposition is
inline const char* failure_words(uint32_t kind) { return kind < KINDS_TOP && KINDS[kind].failure ? KINDS[kind].failure : KINDS[HINT].failure; }
// how many destination words a record has: every step of every scan, else one per element
inline uint64_t dst_words(uint32_t kind, uint32_t count, uint32_t p1) { return kind < KINDS_TOP && KINDS[kind].scan ? (uint64_t)count * p1 : count; }
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
    // the words [off, off + n) as cells a lane reads; in a sparse record 0xffffffff is no entry, and `other`, the array it is paired with
    // (DOT), must have none there either.  -> what is wrong, or nullptr
    auto readable = [&](uint32_t off, uint64_t n, bool sparse, const uint32_t* other) -> const char* {
        for (uint64_t i = 0; i < n; i++) {
            const uint32_t x = P[off + i];
            if (sparse && x == NONE) {
                if (other && other[i] != NONE) return "a product with one operand";
                continue;
            }
            if (x >= cells) return "cell index out of range";
            if (!written.get(x)) return "a cell is read before an earlier record has written it";
        }
        return nullptr;
    };
    // the words at a or b by their role; lim: what an index stays below
    auto operand = [&](Role role, uint32_t off, uint64_t n, uint32_t lim, bool sparse, const uint32_t* other) -> const char* {
        if (role == CELLS) return readable(off, n, sparse, other);
        if (role == INDICES || role == DIGITS)
            for (uint64_t i = 0; i < n; i++)
                if (P[off + i] >= lim && !(role == DIGITS && P[off + i] == NONE)) return role == DIGITS ? "bad decomposition" : "table index out of range";
        return nullptr;
    };
    int col_phase[MAX_ADVICE];
    for (uint32_t c = 0; c < MAX_ADVICE; c++) col_phase[c] = -1;
    uint32_t last_phase = 0;
    for (size_t ri = 0; ri < out.recs.size(); ri++) {
        const Rec& r = out.recs[ri];
        if (!known(r.kind)) return at_rec(ri, r.kind, "unknown kind");
        if (r.count == 0 && r.kind != COMPLEMENT) return at_rec(ri, r.kind, "empty");     // (nothing missing: a complement that writes no cell)
        if (r.phase >= n_phases) return at_rec(ri, r.kind, "phase out of range");
        if (r.phase < last_phase) return at_rec(ri, r.kind, "phases decrease");
        last_phase = r.phase;
        if ((r.kind == INPUT || r.kind == MATMUL) && r.phase != 0) return at_rec(ri, r.kind, "input and matmul records belong to phase 0");
        // the kind's own parameters, and the words it has: n_dst at dst, n_a at a, n_b at b, lim for its indices, n_extra further cells a lane reads
        const KindInfo& K = KINDS[r.kind];
        const uint64_t n_dst = dst_words(r.kind, r.count, r.p1);
        uint64_t n_a = r.count, n_b = 0, n_extra = 0;
        uint32_t lim = 0, extra = 0;
        switch (r.kind) {
        case COPY: case INVZ: break;
        case ADD: case SUB: case MUL: n_b = r.count; break;
        case CONST: lim = n_con; break;
        case INPUT: lim = n_in; break;
        case PARAM: lim = n_par; break;
        case HINT: {                                     // p0 = base, p1 = legs; b: the digit of each element, below p1
            n_b = r.count; lim = r.p1;
            uint64_t bound = 1;
            if (r.p0 < 2 || r.p1 == 0) return at_rec(ri, r.kind, "bad decomposition");
            for (uint32_t t = 0; t < r.p1; t++) {
                if (bound > (((uint64_t)1 << 62) - 1) / r.p0) return at_rec(ri, r.kind, "bad decomposition");     // base^legs < 2^62, without overflow
                bound *= r.p0;
            }
            break;
        }
        case RCIDX: if (r.p1 == 0) return at_rec(ri, r.kind, "zero table column size"); break;
        case DIVC: if (r.p0 == 0) return at_rec(ri, r.kind, "zero divisor"); break;
        case TABLE: case TBLIDX: if (r.p0 >= n_tab) return at_rec(ri, r.kind, "lookup table index out of range"); break;
        case MATMUL:                                     // p0 = kd, p1 = n, count = m * n: a = m * kd, b = kd * n input indices
            if (r.p0 == 0 || r.p1 == 0 || r.count % r.p1 != 0) return at_rec(ri, r.kind, "bad matmul shape");
            n_a = (uint64_t)(r.count / r.p1) * r.p0; n_b = (uint64_t)r.p0 * r.p1; lim = n_in;
            if (!span_ok(r.dst, n_dst) || !span_ok(r.a, n_a) || !span_ok(r.b, n_b)) return at_rec(ri, r.kind, "bad matmul shape");
            break;
        case RLC:                                        // p0 = challenge, p1 = steps, count = scans
            if (r.p0 >= n_chal) return at_rec(ri, r.kind, "challenge index out of range");
            if (r.p1 == 0 || n_dst > P.size()) return at_rec(ri, r.kind, "bad rlc shape");
            n_a = n_dst;
            break;
        case SUMACC: case PRODACC:                       // p0 = operands per step, p1 = steps, count = scans
            if (r.p0 == 0 || r.p1 == 0 || !span_ok(r.dst, n_dst) || !span_ok(r.a, n_dst * r.p0)) return at_rec(ri, r.kind, "bad scan shape");
            n_a = n_dst * r.p0;
            break;
        case GATHER:                                     // p0 = pool offset of the table's cell list, p1 = its length: cells a lane reads
            if (r.p1 == 0) return at_rec(ri, r.kind, "empty gather table");
            if (!span_ok(r.p0, r.p1)) return at_rec(ri, r.kind, "gather table runs past the pool");
            extra = r.p0; n_extra = r.p1;
            break;
        case CLAMP: if ((int32_t)r.p0 > (int32_t)r.p1) return at_rec(ri, r.kind, "bad clamp bounds"); break;
        case SORT: case ARGSORT:                         // p0 = segment length, p1 = mode, count = segments * p0
            if (r.p0 == 0 || r.count % r.p0 != 0 || r.p1 > 1 || r.count > MAX_SORT_COUNT) return at_rec(ri, r.kind, "bad sort shape");
            break;
        case RECIP: {                                    // S = p0 | p1 << 32, b = the constant a zero input takes
            const uint64_t S = (uint64_t)r.p0 | ((uint64_t)r.p1 << 32);
            if (S == 0 || S >= ((uint64_t)1 << 62)) return at_rec(ri, r.kind, "reciprocal scale outside [1, 2^62)");
            if (r.b >= n_con) return at_rec(ri, r.kind, "zero-inverse index past the constants");
            break;
        }
        case ISQRT:
            if (r.p0 == 0) return at_rec(ri, r.kind, "zero square-root scale");
            if (r.p1 != 0) return at_rec(ri, r.kind, "a square-root record with a second parameter");
            break;
        case ARGEXT:                                     // p0 = segment length, p1 = mode, count = segments = destination cells
            n_a = (uint64_t)r.count * r.p0;
            if (r.p0 == 0 || r.p1 > 1 || n_a > MAX_SORT_COUNT || !span_ok(r.dst, n_dst) || !span_ok(r.a, n_a)) return at_rec(ri, r.kind, "bad arg-extremum shape");
            break;
        case SCATTER: {                                  // p0 = elements, p1 = multiplier, b: extent, index cells, source cells, offsets
            n_b = 1 + 3ull * r.p0;
            if (r.p0 == 0 || r.p1 == 0 || r.count > MAX_SORT_COUNT || !span_ok(r.dst, n_dst) || !span_ok(r.a, n_a) || !span_ok(r.b, n_b)) return at_rec(ri, r.kind, "bad scatter shape");
            const uint32_t extent = P[r.b];
            if (extent == 0) return at_rec(ri, r.kind, "bad scatter shape");
            for (uint32_t j = 0; j < r.p0; j++)          // every target of an index inside [0, extent) is a destination: no overflow, both factors are 32-bit
                if ((uint64_t)P[r.b + 1 + 2ull * r.p0 + j] + (uint64_t)(extent - 1) * r.p1 >= r.count) return at_rec(ri, r.kind, "bad scatter shape");
            extra = r.b + 1; n_extra = 2ull * r.p0;      // the index and source cells: ones a lane reads
            break;
        }
        case COMPLEMENT:                                 // p0 = n, p1 = sources, count = n - sources
            n_a = r.p1;
            if (r.p1 > r.p0 || r.count != r.p0 - r.p1 || r.p0 > MAX_SORT_COUNT || !span_ok(r.dst, n_dst) || !span_ok(r.a, n_a)) return at_rec(ri, r.kind, "bad complement shape");
            break;
        case ONEHOT: n_b = r.count; if (r.p0 == 0) return at_rec(ri, r.kind, "zero one-hot classes"); break;     // b: the position of each element
        case DOT:                                        // p0 = products per step, p1 = steps, count = dot products
            if (r.p0 == 0 || r.p1 == 0 || n_dst > P.size() || n_dst * r.p0 > P.size()) return at_rec(ri, r.kind, "bad dot shape");
            n_a = n_b = n_dst * r.p0;
            break;
        }
        // what holds for every kind: the spans inside the pool, every source a cell written earlier or an index below its limit
        const char* bad = readable(extra, n_extra, false, nullptr);
        if (bad) return at_rec(ri, r.kind, bad);
        if (!span_ok(r.dst, n_dst) || !span_ok(r.a, n_a) || (K.b != NOT_POOL && !span_ok(r.b, n_b))) return at_rec(ri, r.kind, "an index array runs past the pool");
        const bool paired = K.sparse && n_b;             // DOT: a product has both operands or none
        if ((bad = operand(K.a, r.a, n_a, lim, K.sparse, paired ? &P[r.b] : nullptr))) return at_rec(ri, r.kind, bad);
        if ((bad = operand(K.b, r.b, n_b, lim, K.sparse, paired ? &P[r.a] : nullptr))) return at_rec(ri, r.kind, bad);
        // destinations after every source of the record: a record never reads what it writes
        for (uint64_t i = 0; i < n_dst; i++) {
            const uint32_t x = P[r.dst + i];
            if (K.sparse && x == NONE) continue;
            if (x >= cells) return at_rec(ri, r.kind, "cell index out of range");
        }
        for (uint64_t i = 0; i < n_dst; i++) {
            const uint32_t x = P[r.dst + i];
            if (K.sparse && x == NONE) continue;
            if (written.get(x)) return at_rec(ri, r.kind, "a cell is written twice");
            written.set(x);
            total++;
        }
        for (uint64_t i = 0; i < n_dst; i++) {
            const uint32_t x = P[r.dst + i];
            if (K.sparse && x == NONE) continue;
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
