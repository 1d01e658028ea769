// The constraint system as data, and the parser of the blob that describes it (ezkl_prover_cs_parse).  Host only: the blob is
// untrusted bytes, and nothing here needs a device.
#pragma once
#include <algorithm>
#include <map>
#include <memory>
#include <set>
#include <utility>
#include "ezkl_hip.hpp"
#include "ezkl_prover.h"
#include "hostfield.hpp"
#include "transcript.hpp"

namespace ezkl_prover {
using ezkl_hip::Error;

// blinding factors: halo2's ConstraintSystem::blinding_factors() = max(3, most queries of one advice column) + 2, carried by the
// blob or derived from the queries; ezkl's circuits give 5 (/root/reference/src/graph/mod.rs:100).  The last blinding+1 rows are unusable.

// ------------------------------------------------------------------ constraint system
enum NodeOp : uint32_t { N_CONST = 0, N_ADV, N_FIX, N_INST, N_CHAL, N_NEG, N_ADD, N_SUB, N_MUL };
struct Node {
    uint32_t op, a, b;
    Fe c;
};
struct Query {
    uint32_t col;
    int32_t rot;
    bool operator<(const Query& o) const { return col != o.col ? col < o.col : rot < o.rot; }
    bool operator==(const Query& o) const { return col == o.col && rot == o.rot; }
};
struct Lookup {
    std::vector<std::vector<uint32_t>> inputs;
    std::vector<uint32_t> table;
};
// MSMs sharded by points (ezkl_prover_cs_set_shard): this rank's SRS handles hold points [lo, hi) only
struct Shard {
    uint32_t lo = 0, hi = 0;          // hi == 0: not sharded
    ezkl_fold_fn fold = nullptr;
    void* user = nullptr;
    ezkl_gather_fn gather = nullptr;  // optional: the quotient sweep sharded by rows (ezkl_prover_cs_set_sweep_gather)
    void* gather_user = nullptr;
    // optional: columns and arguments have owners (ezkl_prover_cs_set_shard_exchange)
    ezkl_allgather_host_fn allgather_host = nullptr;
    ezkl_exchange_fn exchange = nullptr;
    void* xuser = nullptr;
    mutable uint64_t sharded_sweeps = 0;
    mutable uint64_t stats[4] = {0, 0, 0, 0};     // ezkl_prover_cs_shard_stats
    // the SRS handles hold ALL 2^k points on every rank (ezkl_prover_cs_set_shard_full_bases; 288 GB of HBM per GPU: a 2^22 base set
    // with its window tables is 3.5 GB): a commit batch is then divided by COLUMNS -- whole MSMs, which keep the per-call tail of a
    // 2^k-point MSM off the critical path instead of paying it on every 2^k / world slice -- and by point ranges inside a column
    // only when the batch has fewer columns than there are ranks
    bool full_bases = false;
    bool on() const { return hi != 0; }
    // equal power-of-two slices: rank / log2(world) of this one, or false
    bool geometry(uint32_t n, uint32_t& rank, uint32_t& log_world) const {
        const uint32_t len = hi - lo;
        if (!on() || len == 0 || n % len || lo % len) return false;
        const uint32_t world = n / len;
        if (world & (world - 1)) return false;
        rank = lo / len;
        log_world = 0;
        while ((1u << log_world) < world) log_world++;
        return true;
    }
};
// Who does what in one proof.  One rank (or a sharded prover without the exchange callbacks): everything is mine.  Owner mode: witness
// column / argument number i belongs to rank i mod world; only its owner computes, transforms and commits it.
struct Topo {
    uint32_t world = 1, rank = 0, log_world = 0;
    bool owners = false;
    bool mine(size_t i) const { return !owners || (uint32_t)(i % world) == rank; }
    uint32_t owner(size_t i) const { return owners ? (uint32_t)(i % world) : rank; }
};
struct ConstraintSystem {
    uint32_t k = 0, n = 0, n_advice = 0, n_fixed = 0, n_instance = 0, n_challenges = 0;
    std::vector<uint32_t> advice_phase;
    std::vector<Node> nodes;
    std::vector<uint32_t> gates;
    std::vector<std::pair<uint32_t, uint32_t>> perm;      // (kind = N_ADV | N_FIX | N_INST, col)
    std::vector<Lookup> lookups;
    uint32_t usable = 0, degree = 0, chunk = 0, ext_k = 0, n_chunks = 0;
    uint32_t blinding = 0, minimum_degree = 0;           // 0 = derive / none (blob version 1)
    uint32_t n_selectors = 0;                             // halo2 selectors behind the fixed columns: sizes the selector section of vk / pk files
    bool queries_given = false;                           // halo2's order of first query (blob version 2)
    bool advice_by_pointer = false;                       // ezkl_prover_cs_set_advice_by_pointer
    std::vector<uint8_t> unblinded;                       // per advice column: unusable rows hold Blind::default() = 1
    std::array<uint8_t, 32> blob_hash{};                  // keccak256 of the blob: binds gates / lookups / queries into the vk digest
    std::vector<Query> advice_queries, fixed_queries, instance_queries;
    std::vector<uint32_t> deg_memo;
    Shard shard;

    uint32_t deg(uint32_t id) {
        if (deg_memo[id] != UINT32_MAX) return deg_memo[id];
        const Node& nd = nodes[id];
        uint32_t d;
        switch (nd.op) {
        case N_CONST: case N_CHAL: d = 0; break;
        case N_ADV: case N_FIX: case N_INST: d = 1; break;
        case N_NEG: d = deg(nd.a); break;
        case N_ADD: case N_SUB: d = std::max(deg(nd.a), deg(nd.b)); break;
        default: d = deg(nd.a) + deg(nd.b); break;
        }
        return deg_memo[id] = d;
    }
    void collect(uint32_t id, std::set<Query> out[3], std::vector<uint8_t>& seen) const {
        if (seen[id]) return;
        seen[id] = 1;
        const Node& nd = nodes[id];
        if (nd.op == N_ADV || nd.op == N_FIX || nd.op == N_INST) out[nd.op - N_ADV].insert(Query{nd.a, (int32_t)nd.b});
        else if (nd.op == N_NEG) collect(nd.a, out, seen);
        else if (nd.op >= N_ADD) { collect(nd.a, out, seen); collect(nd.b, out, seen); }
    }
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> perm_chunks() const {
        std::vector<std::vector<std::pair<uint32_t, uint32_t>>> out;
        for (size_t i = 0; i < perm.size(); i += chunk) out.emplace_back(perm.begin() + i, perm.begin() + std::min(perm.size(), i + chunk));
        return out;
    }
    void finalize() {
        n = 1u << k;
        deg_memo.assign(nodes.size(), UINT32_MAX);
        uint32_t d = 3;
        for (uint32_t g : gates) d = std::max(d, deg(g));
        for (auto& l : lookups) {                          // l_active * phi * prod(f_j + beta) * (t + beta)
            uint32_t s = 2, tmax = 0;
            for (auto& t : l.inputs) {
                uint32_t m = 0;
                for (uint32_t e : t) m = std::max(m, deg(e));
                s += m;
            }
            for (uint32_t e : l.table) tmax = std::max(tmax, deg(e));
            d = std::max(d, s + tmax);
        }
        degree = d = std::max(d, minimum_degree);
        chunk = d - 2;
        ext_k = k;
        while ((1ull << ext_k) < (uint64_t)n * (d - 1)) ext_k++;
        std::set<Query> qs[3];
        std::vector<uint8_t> seen(nodes.size(), 0);
        for (uint32_t g : gates) collect(g, qs, seen);
        for (auto& pc : perm) qs[pc.first - N_ADV].insert(Query{pc.second, 0});
        for (auto& l : lookups) {
            for (auto& t : l.inputs)
                for (uint32_t e : t) collect(e, qs, seen);
            for (uint32_t e : l.table) collect(e, qs, seen);
        }
        if (queries_given) {                              // must cover what the expressions read, without duplicates
            std::vector<Query>* given[3] = {&advice_queries, &fixed_queries, &instance_queries};
            for (int t = 0; t < 3; t++) {
                std::set<Query> have(given[t]->begin(), given[t]->end());
                if (have.size() != given[t]->size()) throw Error(EZKL_ERR_INVALID, "duplicate query");
                for (auto& q : qs[t])
                    if (!have.count(q)) throw Error(EZKL_ERR_INVALID, "query lists do not cover the expressions");
            }
        } else {
            advice_queries.assign(qs[0].begin(), qs[0].end());
            fixed_queries.assign(qs[1].begin(), qs[1].end());
            instance_queries.assign(qs[2].begin(), qs[2].end());
        }
        if (blinding == 0) {                              // halo2 ConstraintSystem::blinding_factors
            std::map<uint32_t, uint32_t> per_col;
            uint32_t most = 1;
            for (auto& q : advice_queries) most = std::max(most, ++per_col[q.col]);
            blinding = std::max(3u, most) + 2;
        }
        if (blinding + 2 > n) throw Error(EZKL_ERR_INVALID, "no usable rows");
        usable = n - blinding - 1;
        n_chunks = perm.empty() ? 0 : (uint32_t)((perm.size() + chunk - 1) / chunk);
    }
};

struct Reader {
    const uint8_t* p;
    size_t left;
    uint32_t u32() {
        if (left < 4) throw Error(EZKL_ERR_INVALID, "constraint system blob truncated");
        uint32_t v;
        std::memcpy(&v, p, 4);
        p += 4; left -= 4;
        return v;
    }
    void bytes(void* out, size_t m) {
        if (left < m) throw Error(EZKL_ERR_INVALID, "constraint system blob truncated");
        std::memcpy(out, p, m);
        p += m; left -= m;
    }
};
inline void invalid(bool cond, const char* what) {
    if (cond) throw Error(EZKL_ERR_INVALID, what);
}
inline std::unique_ptr<ConstraintSystem> parse_cs(const void* blob, size_t len) {
    Reader r{(const uint8_t*)blob, len};
    invalid(r.u32() != 0x53435a45u, "bad magic");
    const uint32_t version = r.u32();
    invalid(version != 1 && version != 2, "unsupported version");
    auto cs = std::make_unique<ConstraintSystem>();
    cs->blob_hash = keccak256((const uint8_t*)blob, len);
    cs->k = r.u32(); cs->n_advice = r.u32(); cs->n_fixed = r.u32(); cs->n_instance = r.u32(); cs->n_challenges = r.u32();
    invalid(cs->k < 4 || cs->k > 28, "k out of range");
    invalid(cs->n_advice > (1u << 16) || cs->n_fixed > (1u << 16) || cs->n_instance > (1u << 16) || cs->n_challenges > (1u << 16), "column count out of range");
    for (uint32_t i = 0; i < cs->n_advice; i++) {
        cs->advice_phase.push_back(r.u32());
        invalid(cs->advice_phase.back() > 1, "advice phase must be 0 or 1");
    }
    cs->unblinded.assign(cs->n_advice, 0);
    if (version >= 2) {
        cs->blinding = r.u32();
        cs->minimum_degree = r.u32();
        invalid(cs->blinding > 64 || cs->minimum_degree > 64, "blinding / minimum degree out of range");
        const uint32_t nu = r.u32();
        invalid((size_t)nu * 4 > r.left, "unblinded list truncated");
        for (uint32_t i = 0; i < nu; i++) {
            const uint32_t c = r.u32();
            invalid(c >= cs->n_advice, "unblinded column out of range");
            cs->unblinded[c] = 1;
        }
        cs->n_selectors = r.u32();
        invalid(cs->n_selectors > (1u << 20), "selector count out of range");
    }
    const uint32_t nn = r.u32();
    invalid((size_t)nn * 48 > r.left, "node table truncated");
    for (uint32_t i = 0; i < nn; i++) {
        Node nd;
        nd.op = r.u32(); nd.a = r.u32(); nd.b = r.u32();
        r.u32();
        r.bytes(nd.c.v.data(), 32);
        invalid(nd.op > N_MUL, "bad node op");
        if (nd.op == N_CONST) invalid(cmp(nd.c.v, FR.p) >= 0, "non-canonical constant");
        if (nd.op == N_ADV) invalid(nd.a >= cs->n_advice, "advice column out of range");
        if (nd.op == N_FIX) invalid(nd.a >= cs->n_fixed, "fixed column out of range");
        if (nd.op == N_INST) invalid(nd.a >= cs->n_instance, "instance column out of range");
        if (nd.op == N_CHAL) invalid(nd.a >= cs->n_challenges, "challenge index out of range");
        if (nd.op >= N_NEG) invalid(nd.a >= i, "child must precede parent");
        if (nd.op >= N_ADD) invalid(nd.b >= i, "child must precede parent");
        cs->nodes.push_back(nd);
    }
    auto node_list = [&](std::vector<uint32_t>& out) {
        const uint32_t m = r.u32();
        invalid((size_t)m * 4 > r.left, "list truncated");
        for (uint32_t i = 0; i < m; i++) {
            out.push_back(r.u32());
            invalid(out.back() >= nn, "node id out of range");
        }
    };
    node_list(cs->gates);
    const uint32_t np = r.u32();
    invalid((size_t)np * 8 > r.left, "permutation list truncated");
    for (uint32_t i = 0; i < np; i++) {
        uint32_t kind = r.u32(), col = r.u32();
        invalid(kind < N_ADV || kind > N_INST, "bad permutation column kind");
        invalid(col >= (kind == N_ADV ? cs->n_advice : kind == N_FIX ? cs->n_fixed : cs->n_instance), "permutation column out of range");
        cs->perm.emplace_back(kind, col);
    }
    const uint32_t nl = r.u32();
    for (uint32_t i = 0; i < nl; i++) {
        Lookup l;
        const uint32_t ni = r.u32();
        invalid(ni == 0 || (size_t)ni * 4 > r.left, "lookup without inputs");
        for (uint32_t j = 0; j < ni; j++) {
            l.inputs.emplace_back();
            node_list(l.inputs.back());
            invalid(l.inputs.back().empty(), "empty lookup tuple");
        }
        node_list(l.table);
        for (auto& t : l.inputs) invalid(t.size() != l.table.size(), "lookup arity mismatch");
        cs->lookups.push_back(std::move(l));
    }
    if (version >= 2) {
        cs->queries_given = r.u32() != 0;
        if (cs->queries_given) {
            std::vector<Query>* lists[3] = {&cs->advice_queries, &cs->fixed_queries, &cs->instance_queries};
            const uint32_t limits[3] = {cs->n_advice, cs->n_fixed, cs->n_instance};
            for (int t = 0; t < 3; t++) {
                const uint32_t m = r.u32();
                invalid((size_t)m * 8 > r.left, "query list truncated");
                for (uint32_t i = 0; i < m; i++) {
                    Query q;
                    q.col = r.u32();
                    q.rot = (int32_t)r.u32();
                    invalid(q.col >= limits[t], "query column out of range");
                    lists[t]->push_back(q);
                }
            }
        }
    }
    invalid(r.left != 0, "trailing bytes");
    cs->finalize();
    return cs;
}

}  // namespace ezkl_prover
