"""A halo2-shaped KZG/SHPLONK prover driving the HIP kernels end to end.

This is the host side of `create_proof` ([UPSTREAM] halo2_proofs::plonk::prover, called from
/root/reference/src/pfsys/mod.rs:456-463) restated in Python over a small column-handle backend interface: every
O(n) step (commitments = MSM, iNTT / coset NTT, the quotient sweep, grand products, polynomial evaluation, SHPLONK
quotients) runs in the kernels of libezkl_hip.so on resident columns; the host owns the transcript, the RNG and the
scalar glue, exactly the split the north-star describes.  Round order follows SURVEY.md §3.1: advice commits ->
beta, gamma -> permutation products -> random poly -> y -> quotient pieces -> x -> evaluations -> SHPLONK.

Compatibility with the zkonduit halo2 fork (its source is not on disk): the proof format is the EvmTranscript layout of the
reference's proofs (points 64 B BE, scalars 32 B BE), and the protocol is pinned on the one executable piece of halo2 the reference
ships -- the compiled Solidity verifier tests/assets/wasm.code: with its verifying-key constants replaced by this key's, the
reference's bytecode derives the same eight challenges, evaluates the same 200 quotient terms and ACCEPTS the proofs written here
(tests/test_evm_verifier.py; NOTEBOOK.md §2.1).  What stays unpinned is the 32-byte vk digest (halo2 hashes the Debug text of its
constraint system); this module binds keccak256 of the serialised constraint system + the commitments in its place.

Covered: custom gates, the permutation argument (chunked), mv-lookup (logUp) arguments with theta-compressed tuples,
instance columns (hashed, not committed; evaluated by the verifier), second-phase advice with post-commitment challenges.
"""
import numpy as np
from .transcript import EvmTranscript, keccak256, R
from . import backend as _b

ROOT = pow(7, (R - 1) >> 28, R)
DELTA = pow(7, 1 << 28, R)
ZETA = 0x30644e72e131a029048b6e193fd84104cc37a73fec2bc5e9b8ca0b2d36636f23
MONT = 1 << 256
RINV = pow(MONT, -1, R)
Q = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
QINV = pow(MONT, -1, Q)
BLINDING = 5                        # as in ezkl (src/graph/mod.rs:100): the last BLINDING+1 rows are unusable


def to_mont(x):
    return np.frombuffer((x % R * MONT % R).to_bytes(32, "little"), np.uint64).copy()


def from_mont(a):
    return int.from_bytes(np.ascontiguousarray(a, np.uint64).tobytes(), "little") * RINV % R


def point_to_ints(p):
    """affine 8 x u64 Montgomery -> (x, y) standard ints, identity -> None"""
    b = np.ascontiguousarray(p, np.uint64).tobytes()
    x, y = int.from_bytes(b[:32], "little") * QINV % Q, int.from_bytes(b[32:], "little") * QINV % Q
    return None if (x == 0 and y == 0) else (x, y)


# ------------------------------------------------------------------ expressions
class Expr:
    """polynomial expression over column queries; node = (op, ...)"""

    def __init__(self, node):
        self.node = node

    def _w(self, o):
        return o if isinstance(o, Expr) else Expr(("const", int(o) % R))

    def __add__(self, o): return Expr(("add", self, self._w(o)))
    def __radd__(self, o): return self._w(o) + self
    def __sub__(self, o): return Expr(("sub", self, self._w(o)))
    def __rsub__(self, o): return self._w(o) - self
    def __mul__(self, o): return Expr(("mul", self, self._w(o)))
    def __rmul__(self, o): return self._w(o) * self
    def __neg__(self): return Expr(("neg", self))


def adv(col, rot=0): return Expr(("adv", col, rot))
def fix(col, rot=0): return Expr(("fix", col, rot))
def inst(col, rot=0): return Expr(("inst", col, rot))
def chal(idx): return Expr(("chal", idx))
def const(v): return Expr(("const", int(v) % R))


def degree(e):
    op = e.node[0]
    if op in ("const", "chal"): return 0
    if op in ("adv", "fix", "inst"): return 1
    if op == "neg": return degree(e.node[1])
    if op in ("add", "sub"): return max(degree(e.node[1]), degree(e.node[2]))
    return degree(e.node[1]) + degree(e.node[2])


def queries(e, out):
    op = e.node[0]
    if op in ("adv", "fix", "inst"):
        out.add((op, e.node[1], e.node[2]))
    elif op not in ("const", "chal"):
        for c in e.node[1:]:
            queries(c, out)
    return out


def evaluate(e, q):
    """verifier side: q(kind, col, rot) -> int  (kind "chal": q("chal", idx, 0))"""
    op = e.node[0]
    if op == "const": return e.node[1]
    if op == "chal": return q("chal", e.node[1], 0)
    if op in ("adv", "fix", "inst"): return q(op, e.node[1], e.node[2])
    if op == "neg": return (-evaluate(e.node[1], q)) % R
    a, b = evaluate(e.node[1], q), evaluate(e.node[2], q)
    return (a + b) % R if op == "add" else (a - b) % R if op == "sub" else a * b % R


def lower(e, prog, col_index, memo):
    """emit the expression into a GraphProgram; col_index(kind, col) -> column slot of the program"""
    key = id(e)
    if key in memo: return memo[key]
    op = e.node[0]
    if op == "const": r = prog.constant(to_mont(e.node[1]))
    elif op == "chal": r = col_index("chal", e.node[1])
    elif op in ("adv", "fix", "inst"): r = prog.column(col_index(op, e.node[1]), e.node[2])
    elif op == "neg": r = prog.calc("negate", lower(e.node[1], prog, col_index, memo))
    else: r = prog.calc(op, lower(e.node[1], prog, col_index, memo), lower(e.node[2], prog, col_index, memo))
    memo[key] = r
    return r


class ConstraintSystem:
    def __init__(self, k, n_advice, n_fixed, gates, permutation_columns, lookups=(), n_instance=0, advice_phase=None, n_challenges=0,
                 query_order=None, blinding=None, minimum_degree=None, unblinded=(), n_selectors=0):
        """lookups: [(input_tuples, table_tuple)]: every input tuple (list of Expr) of a lookup must appear as a row of
        the table tuple (list of Expr of the same arity) on the usable rows -- the mv-lookup (logUp) argument the
        zkonduit halo2 fork uses (cargo feature `mv-lookup`, /root/reference/Cargo.toml:255).
        query_order: (advice, fixed, instance) lists of (column, rotation) in halo2's order of first query (halo2_cs.py); without
        it the queries are collected from the expressions and sorted.  blinding: halo2's cs.blinding_factors() (computed from
        the advice queries when omitted: max(3, most queries of one advice column) + 2; ezkl's circuits give 5,
        src/graph/mod.rs:100).  minimum_degree: set by halo2's chunk_lookups.  unblinded: advice columns whose unusable rows
        hold Blind::default() = 1 instead of randomness (src/circuit/modules/polycommit.rs:57-61, src/tensor/var.rs:73-108)."""
        self.k, self.n = k, 1 << k
        self.n_advice, self.n_fixed, self.n_instance = n_advice, n_fixed, n_instance
        # second-phase advice (ezkl's Freivalds einsum, src/circuit/ops/chip/einsum/mod.rs:67-76,716): columns with phase 1 are
        # committed after `n_challenges` challenges have been squeezed from the first-phase commitments
        self.advice_phase = list(advice_phase) if advice_phase is not None else [0] * n_advice
        self.n_challenges = n_challenges
        self.gates = list(gates)
        self.perm = list(permutation_columns)             # [("adv"|"fix"|"inst", col)]
        self.lookups = [([list(t) for t in ins], list(tab)) for ins, tab in lookups]
        self.unblinded = sorted(set(unblinded))
        self.n_selectors = n_selectors                    # halo2 selectors behind the fixed columns (sizes the selector section of key files)
        self.minimum_degree = minimum_degree
        d = max([degree(g) for g in self.gates] + [3])
        for ins, tab in self.lookups:                     # l_active * phi * prod(f_j + beta) * (t + beta)
            d = max(d, 2 + sum(max(degree(e) for e in t) for t in ins) + max(degree(e) for e in tab))
        self.degree = max(d, minimum_degree or 1)
        self.chunk = self.degree - 2
        self.ext_k = k
        while (1 << self.ext_k) < self.n * (self.degree - 1):
            self.ext_k += 1
        qs = set()
        for g in self.gates:
            queries(g, qs)
        for kind, c in self.perm:
            qs.add((kind, c, 0))
        for ins, tab in self.lookups:
            for t in ins + [tab]:
                for e in t:
                    queries(e, qs)
        if query_order is not None:
            self.advice_queries, self.fixed_queries, self.instance_queries = [[(int(c), int(r)) for c, r in q] for q in query_order]
            have = {("adv", c, r) for c, r in self.advice_queries} | {("fix", c, r) for c, r in self.fixed_queries} | {("inst", c, r) for c, r in self.instance_queries}
            assert qs <= have, "query lists do not cover the expressions: %s" % sorted(qs - have)[:4]
            for q in (self.advice_queries, self.fixed_queries, self.instance_queries):
                assert len(set(q)) == len(q), "duplicate query"
        else:
            self.advice_queries = sorted((c, r) for kd, c, r in qs if kd == "adv")
            self.fixed_queries = sorted((c, r) for kd, c, r in qs if kd == "fix")
            self.instance_queries = sorted((c, r) for kd, c, r in qs if kd == "inst")
        self.queries_given = query_order is not None
        if blinding is None:                              # halo2 ConstraintSystem::blinding_factors
            per_col = {}
            for c, _ in self.advice_queries:
                per_col[c] = per_col.get(c, 0) + 1
            blinding = max(3, max(per_col.values(), default=1)) + 2
        self.blinding = blinding
        self.usable = self.n - blinding - 1               # row index of l_last; rows [0, usable) carry the witness
        assert self.usable > 0
        self.n_chunks = -(-len(self.perm) // self.chunk) if self.perm else 0

    def perm_chunks(self):
        return [self.perm[i:i + self.chunk] for i in range(0, len(self.perm), self.chunk)]


def omega(k): return pow(ROOT, 1 << (28 - k), R)


# ------------------------------------------------------------------ GPU backend (column handles = DeviceBuffer)
class GpuBackend:
    """every column is a resident HBM buffer; scalars cross the ABI as 32-byte Montgomery values"""
    name = "hip"

    def __init__(self, params_g, params_g_lagrange, k):
        self.k, self.n = k, 1 << k
        self.g = _b.Bases(params_g)
        self.gl = _b.Bases(params_g_lagrange)
        self._dom = {}
        self._zpow = {}

    def dom(self, degree):
        if degree not in self._dom:
            self._dom[degree] = _b.EvaluationDomain(degree, self.k)
        return self._dom[degree]

    def upload(self, a): return _b.DeviceBuffer.from_numpy(np.ascontiguousarray(a, np.uint64))
    def download(self, h, n): return h.to_numpy()[: 4 * n].reshape(n, 4)
    def clone(self, h):
        o = _b.DeviceBuffer(h.nbytes)
        _b.vec_scale(h.ptr, to_mont(1), o.ptr, h.nbytes // 32)
        return o
    def commit_lagrange(self, hs): return [point_to_ints(p) for p in _b.msm_g1_batch_dev(self.gl, [h.ptr for h in hs], self.n)]
    def commit(self, hs): return [point_to_ints(p) for p in _b.msm_g1_batch_dev(self.g, [h.ptr for h in hs], self.n)]
    def lagrange_to_coeff(self, h):
        o = self.clone(h)
        d = self.dom(3)
        _b.ntt_dev(o.ptr, self.k, d.omega_inv, inverse=True)
        return o
    def coeff_to_extended(self, h, ext_k):
        o = _b.DeviceBuffer(32 << ext_k)
        _b.coset_ntt_dev(h.ptr, o.ptr, self.k, ext_k, inverse=False)
        return o
    def extended_to_coeff(self, h, ext_k):
        _b.coset_ntt_dev(h.ptr, h.ptr, self.k, ext_k, inverse=True)
        return h
    def divide_by_vanishing(self, h, ext_k): _b.divide_by_vanishing_dev(h.ptr, self.k, ext_k)
    def eval_program(self, prog, cols, challenges, out): prog.evaluate_h([c.ptr for c in cols], [to_mont(c) for c in challenges], out.ptr)
    def zeros(self, n):
        o = _b.DeviceBuffer(32 * n)
        _b.vec_fill(o.ptr, np.zeros(4, np.uint64), n)
        return o
    def eval_poly(self, h, n, x, offset=0): return from_mont(_b.eval_polynomial(h.ptr + 32 * offset, n, to_mont(x)))
    def slice_copy(self, h, offset, n):
        o = _b.DeviceBuffer(32 * n)
        _b.vec_scale(h.ptr + 32 * offset, to_mont(1), o.ptr, n)
        return o
    def axpy(self, acc, s, h, n):
        """acc += s * h over n elements"""
        t = _b.DeviceBuffer(32 * n)
        _b.vec_scale(h.ptr, to_mont(s), t.ptr, n)
        _b.vec_op("add", acc.ptr, t.ptr, acc.ptr, n)
    def sub_low(self, h, coeffs):
        """h[i] -= coeffs[i] for the few lowest coefficients"""
        m = len(coeffs)
        t = self.upload(np.stack([to_mont(c) for c in coeffs]))
        _b.vec_op("sub", h.ptr, t.ptr, h.ptr, m)
    def scale(self, h, s, n): _b.vec_scale(h.ptr, to_mont(s), h.ptr, n)
    def permutation_product(self, value_cols, sigma_cols, beta, gamma, first_index, z0, omega_col):
        return _b.permutation_grand_product(self.k, [c.ptr for c in value_cols], [c.ptr for c in sigma_cols], to_mont(beta), to_mont(gamma),
                                            omega_col=omega_col, first_column_index=first_index, z0=None if z0 is None else to_mont(z0))
    def omega_powers(self): return _b.omega_powers_column(self.k)
    def lookup_multiplicity(self, inputs, table, usable):
        m, missing = _b.lookup_multiplicity([h.ptr for h in inputs], table.ptr, self.n, usable)
        return m, missing
    def lookup_grand_sum(self, inputs, table, m, beta):
        return _b.lookup_grand_sum(self.k, [h.ptr for h in inputs], table.ptr, m.ptr, to_mont(beta))
    def set_rows(self, h, start, mont_rows):
        """overwrite rows [start, start+len) (blinding rows) with host values (Montgomery (m,4) array)"""
        _b.memcpy_h2d(h.ptr + 32 * start, np.ascontiguousarray(mont_rows, np.uint64))
    def get_row(self, h, i): return from_mont(_b.memcpy_d2h(h.ptr + 32 * i, 32).view(np.uint64))
    def kate_div(self, h, z, n):
        """q(X) = p(X) / (X - z) in place (halo2's kate_division)"""
        _b.kate_division(h.ptr, to_mont(z), h.ptr, n)
        return h


class Rng:
    """prover randomness (blinding rows, the vanishing argument's random polynomial), uniform on [0, r) by rejection
    sampling.  Unseeded = OS entropy (the reference's OsRng, src/pfsys/mod.rs:436-439); seeded = its `det-prove` feature
    (tests only: a deterministic stream, NOT cryptographic)."""

    def __init__(self, seed=None):
        self.g = None if seed is None else np.random.default_rng(seed)

    def _raw(self, m):
        if self.g is None:
            import os
            return np.frombuffer(os.urandom(32 * m), np.uint64).reshape(m, 4).copy()
        return self.g.bit_generator.random_raw(4 * m).astype(np.uint64, copy=False).reshape(m, 4)

    def vec(self, m):
        out = np.empty((m, 4), np.uint64)
        have = 0
        top, rest = np.uint64(R >> 192), [np.uint64((R >> s) & 0xffffffffffffffff) for s in (128, 64, 0)]
        while have < m:
            a = self._raw(m - have + 8)
            a[:, 3] &= np.uint64((1 << 62) - 1)      # 254 bits; accept a < r (limb-wise comparison, most significant first)
            lt = a[:, 3] < top
            eq = a[:, 3] == top
            for limb, rv in zip((2, 1, 0), rest):
                lt |= eq & (a[:, limb] < rv)
                eq &= a[:, limb] == rv
            a = a[lt][: m - have]
            out[have:have + len(a)] = a
            have += len(a)
        return out


class _SharedEval:
    """marks an owned polynomial whose evaluations are taken from the all_gathered list (same consumption order on every rank)"""
    _shared_eval = True

    def __init__(self, h):
        self.h = h


class ColumnShardMixin:
    """NTTs sharded by COLUMNS over the ranks of a torch.distributed group, on top of a backend whose MSMs are
    sharded by points and whose sweep is sharded by rows.  Requires of the backend: download / upload / window / eval_rows /
    gather_rows (the row-shard primitives) and eval_poly / zeros / axpy.  Replicated data (the key's fixed / sigma columns, the
    witness VALUES every rank receives) are owned by everyone: in SHPLONK's partial sums they count on rank (index % world)."""

    def _dist_init(self, dist, device):
        self.dist, self.device = dist, device
        self.world = dist.get_world_size() if dist is not None and dist.is_initialized() else 1
        self.rank = dist.get_rank() if self.world > 1 else 0
        self.sharded_ntt_columns = 0

    def owner_of(self, index):
        return index % self.world

    def lagrange_to_coeff(self, h):
        self.sharded_ntt_columns += 1
        return super().lagrange_to_coeff(h)

    def eval_program_sharded(self, prog, cols, owners, challenges, out):
        """cols[i] is None where another rank owns slot i; owners[i] = owning rank, -1 = resident on every rank"""
        from . import dist as D
        world, rank = self.world, self.rank
        ne, m = 1 << prog.ext_k, world.bit_length() - 1
        assert (1 << m) == world and m <= prog.k, "the row-sharded sweep needs a power-of-two world"
        sub, queries = prog.row_sharded(m)
        lo, hi = D.shard_range(ne, rank, world)
        exq = [(c, s) for c, s in queries if owners[c] >= 0]
        owned = {c: np.asarray(self.download(cols[c], ne)) for c in {c for c, _ in exq} if owners[c] == rank}
        got = D.reshard_columns_to_rows(owned, exq, ne, self.dist, self.device, owner=lambda c: owners[c])
        handles = []
        for c, s in queries:
            if owners[c] >= 0:
                handles.append(self.upload(got[(c, s)]))
            else:
                handles.append(self.window(cols[c], (lo + s) % ne, hi - lo, ne))
        self.eval_rows(sub, handles, challenges, out, lo, hi)
        self.gather_rows(out, lo, hi, ne)
        self.sharded_sweeps = getattr(self, "sharded_sweeps", 0) + 1

    def eval_by_owner(self, wanted, n):
        """wanted: [(poly handle or None, owner, point)] in the same order on every rank -> the evaluations, on every rank"""
        from . import dist as D
        mine = [self.eval_poly(h, n, pt) if o == self.rank else 0 for h, o, pt in wanted]
        allv = D.allgather_ints(mine, self.dist, self.device)
        return [allv[o][i] for i, (_, o, _) in enumerate(wanted)]

    def sum_over_ranks(self, h, n):
        from . import dist as D
        parts = D.allgather_array(np.asarray(self.download(h, n)), self.dist, self.device)
        acc = self.upload(parts[0])
        for p_ in parts[1:]:
            self.axpy(acc, 1, self.upload(p_), n)
        return acc


class DistGpuBackend(ColumnShardMixin, GpuBackend):
    """BASELINE configs[3]: the MSMs of a proof sharded across the GPUs of a node.  Every rank runs
    the same deterministic prover on replicated columns but holds only its contiguous slice of the SRS (base-set memory
    and MSM work divide by the world size); each commit batch ends with ONE all_gather of the 64-byte partials (RCCL
    over xGMI) and a host fold, so all ranks derive identical transcripts.  NTTs / the sweep stay replicated here."""
    name = "hip-dist"

    def __init__(self, params_g, params_g_lagrange, k, dist, device, shard_columns=False):
        from . import dist as D
        self.D = D
        self._dist_init(dist, device)
        world, rank = self.world, self.rank
        if not (shard_columns and world > 1 and world & (world - 1) == 0):
            self.owner_of = None                     # NTTs replicated (MSMs by points + sweep by rows only)
        self.lo, self.hi = D.shard_range(1 << k, rank, world)
        self.k, self.n = k, 1 << k
        self.g = _b.Bases(np.ascontiguousarray(params_g[self.lo:self.hi]))
        self.gl = _b.Bases(np.ascontiguousarray(params_g_lagrange[self.lo:self.hi]))
        self._dom, self._zpow = {}, {}

    def _commit(self, bases, hs):
        part = _b.msm_g1_batch_dev(bases, [h.ptr + 32 * self.lo for h in hs], self.hi - self.lo)
        full = self.D.fold_columns(self.D.allgather_points(part, self.dist, self.device))
        return [point_to_ints(p) for p in full]

    def commit_lagrange(self, hs): return self._commit(self.gl, hs) if hs else []
    def commit(self, hs): return self._commit(self.g, hs) if hs else []

    SWEEP_MIN_ROWS = 1 << 14

    # the row-shard primitives of ColumnShardMixin on resident buffers
    def window(self, h, start, length, total):
        if start + length <= total:
            return _b.DeviceView(h.ptr + 32 * start, 32 * length, h)
        w, first = _b.DeviceBuffer(32 * length), total - start
        one = to_mont(1)
        _b.vec_scale(h.ptr + 32 * start, one, w.ptr, first)
        _b.vec_scale(h.ptr, one, w.ptr + 32 * first, length - first)
        return w
    def eval_rows(self, sub, handles, challenges, out, lo, hi):
        sub.evaluate_h([h.ptr for h in handles], [to_mont(c) for c in challenges], out.ptr + 32 * lo)
    def gather_rows(self, out, lo, hi, total):
        self.D.allgather_rows(out, lo, hi, total, self.dist, self.device)

    def eval_program(self, prog, cols, challenges, out):
        """The quotient sweep sharded by ROWS: this rank evaluates rows [lo, hi) of the extended domain with the
        program rewritten per shard (GraphProgram.row_sharded: every (column, rotation) read becomes a window of the resident
        column -- an offset pointer, or a stitched copy when the window wraps around the domain) and the ranks all_gather their
        rows of h.  The columns are replicated here (the NTTs are not sharded yet), so there is no column exchange."""
        world = self.dist.get_world_size() if self.dist is not None and self.dist.is_initialized() else 1
        ne, m = 1 << prog.ext_k, world.bit_length() - 1
        if world == 1 or (1 << m) != world or m > prog.k or ne < self.SWEEP_MIN_ROWS:
            return super().eval_program(prog, cols, challenges, out)
        rank = self.dist.get_rank()
        sub, queries = prog.row_sharded(m)
        lo, hi = self.D.shard_range(ne, rank, world)
        one, ptrs, keep = to_mont(1), [], []
        for c, start, ln in self.D.row_windows(queries, ne, rank, world):
            if start + ln <= ne:
                ptrs.append(cols[c].ptr + 32 * start)
            else:
                w, first = _b.DeviceBuffer(32 * ln), ne - start
                _b.vec_scale(cols[c].ptr + 32 * start, one, w.ptr, first)
                _b.vec_scale(cols[c].ptr, one, w.ptr + 32 * first, ln - first)
                keep.append(w)
                ptrs.append(w.ptr)
        sub.evaluate_h(ptrs, [to_mont(c) for c in challenges], out.ptr + 32 * lo)
        self.D.allgather_rows(out, lo, hi, ne, self.dist, self.device)
        self.sharded_sweeps = getattr(self, "sharded_sweeps", 0) + 1


# ------------------------------------------------------------------ keygen
class ProvingKey:
    pass


def keygen(cs, backend, fixed_values, copies):
    """fixed_values: list of (n,4) Montgomery arrays; copies: list of ((colpos, row), (colpos, row)) equalities where
    colpos indexes cs.perm.  Returns the proving key (resident polys / cosets) and the verifying key."""
    n, k = cs.n, cs.k
    w = omega(k)
    pk = ProvingKey()
    pk.cs = cs
    pk.fixed_values = [backend.upload(v) for v in fixed_values]
    pk.fixed_polys = [backend.lagrange_to_coeff(h) for h in pk.fixed_values]
    pk.fixed_cosets = [backend.coeff_to_extended(h, cs.ext_k) for h in pk.fixed_polys]
    # permutation: cycle structure over (colpos, row) cells; sigma[colpos][row] = delta^colpos' * omega^row'
    m = len(cs.perm)
    # cells are numbered c * n + r; `nxt` is the cycle successor, `root` a cycle label, `size` the cycle length
    nxt = np.arange(m * n, dtype=np.int64)
    root = np.arange(m * n, dtype=np.int64)
    size = np.ones(m * n, dtype=np.int64)
    for (ca, ra), (cb, rb) in copies:
        a, b2 = ca * n + ra, cb * n + rb
        if root[a] == root[b2]:
            continue
        if size[root[a]] < size[root[b2]]:
            a, b2 = b2, a
        ra_, rb_ = root[a], root[b2]
        size[ra_] += size[rb_]
        cur = b2
        while True:                                   # relabel the smaller cycle
            root[cur] = ra_
            cur = nxt[cur]
            if cur == b2:
                break
        nxt[a], nxt[b2] = nxt[b2], nxt[a]
    # sigma[c][r] = delta^c' * omega^r' for (c', r') = mapping[(c, r)]: gather from the m columns delta^c * omega^row
    pk.omega_col = backend.omega_powers()
    if pk.omega_col is not None:
        wcol = backend.download(pk.omega_col, n).copy()
    else:
        wcol = np.empty((n, 4), np.uint64)
        acc = 1
        for i in range(n):
            wcol[i] = to_mont(acc)
            acc = acc * w % R
    dcols = []
    for c in range(m):
        h = backend.upload(wcol)
        backend.scale(h, pow(DELTA, c, R), n)
        dcols.append(backend.download(h, n).copy())
    mc = (nxt // n).reshape(m, n)
    mr = (nxt % n).reshape(m, n)
    dstack = np.stack(dcols) if m else np.zeros((0, n, 4), np.uint64)
    sig = [dstack[mc[c], mr[c]] for c in range(m)]
    pk.sigma_values = [backend.upload(s) for s in sig]
    pk.sigma_polys = [backend.lagrange_to_coeff(h) for h in pk.sigma_values]
    pk.sigma_cosets = [backend.coeff_to_extended(h, cs.ext_k) for h in pk.sigma_polys]
    # l0, l_last, l_active_row
    def lag(rows):
        v = np.zeros((n, 4), np.uint64)
        v[list(rows)] = to_mont(1)
        return backend.coeff_to_extended(backend.lagrange_to_coeff(backend.upload(v)), cs.ext_k)
    pk.l0 = lag([0])
    pk.l_last = lag([cs.usable])
    pk.l_active = lag(range(cs.usable))
    # the identity column X on the extended coset: zeta * omega_ext^i, as a resident column (from coefficients [0, 1, 0...])
    xcoef = np.zeros((n, 4), np.uint64)
    xcoef[1] = to_mont(1)
    pk.x_coset = backend.coeff_to_extended(backend.upload(xcoef), cs.ext_k)
    vk = VerifyingKey()
    vk.cs = cs
    vk.fixed_commitments = backend.commit(pk.fixed_polys) if pk.fixed_polys else []
    vk.sigma_commitments = backend.commit(pk.sigma_polys) if pk.sigma_polys else []
    vk.digest = vk_digest(vk)
    pk.vk = vk
    return pk, vk


class VerifyingKey:
    pass


def export_keys(pk, backend):
    """the proving / verifying key in the raw-bytes layout of halo2's ProvingKey::write (the format of the reference's
    pk.key / vk.key, SURVEY.md §8(c) item 3, written by /root/reference/src/pfsys/mod.rs:638-683 save_pk / save_vk):
    returns (vk_bytes, pk_bytes).  The selector section holds cs.n_selectors bit-packed rows (pk.selectors, zero when the
    circuit was described with plain fixed columns)."""
    from . import codecs
    cs = pk.cs
    def pt(p):
        x, y = (0, 0) if p is None else p
        return np.frombuffer((x * MONT % Q).to_bytes(32, "little") + (y * MONT % Q).to_bytes(32, "little"), np.uint64)
    vk = dict(k=cs.k, compress_selectors=True,
              fixed_commitments=np.stack([pt(p) for p in pk.vk.fixed_commitments]) if pk.vk.fixed_commitments else np.zeros((0, 8), np.uint64),
              permutation_commitments=np.stack([pt(p) for p in pk.vk.sigma_commitments]) if pk.vk.sigma_commitments else np.zeros((0, 8), np.uint64),
              selectors=getattr(pk, "selectors", None) if getattr(pk, "selectors", None) is not None else np.zeros((cs.n_selectors, cs.n), bool))
    ne = 1 << cs.ext_k
    dl = lambda h, m: np.array(backend.download(h, m), np.uint64, copy=True)
    d = dict(vk=vk, l0=dl(pk.l0, ne), l_last=dl(pk.l_last, ne), l_active_row=dl(pk.l_active, ne),
             fixed_values=[dl(h, cs.n) for h in pk.fixed_values], fixed_polys=[dl(h, cs.n) for h in pk.fixed_polys],
             fixed_cosets=[dl(h, ne) for h in pk.fixed_cosets], permutations=[dl(h, cs.n) for h in pk.sigma_values],
             perm_polys=[dl(h, cs.n) for h in pk.sigma_polys], perm_cosets=[dl(h, ne) for h in pk.sigma_cosets])
    return codecs.write_vk(vk), codecs.write_pk(d)


_OPS = {"const": 0, "adv": 1, "fix": 2, "inst": 3, "chal": 4, "neg": 5, "add": 6, "sub": 7, "mul": 8}
_KINDS = {"adv": 1, "fix": 2, "inst": 3}


def serialize_cs(cs):
    """ConstraintSystem -> the EZCS blob of include/ezkl_prover.h, version 2 (expression DAG with shared sub-expressions kept
    shared; blinding factors, minimum degree, unblinded columns and halo2's query order carried explicitly).  The blob is the
    canonical description of the circuit: its hash is what the vk digest binds."""
    import struct
    nodes, ids = [], {}

    def visit(e):
        stack = [e]
        while stack:                                   # iterative: gate expressions of wide circuits are deep
            cur = stack[-1]
            if id(cur) in ids:
                stack.pop(); continue
            op = cur.node[0]
            kids = [c for c in cur.node[1:] if isinstance(c, Expr)] if op in ("neg", "add", "sub", "mul") else []
            pend = [c for c in kids if id(c) not in ids]
            if pend:
                stack.extend(pend); continue
            a = b = 0
            cst = bytes(32)
            if op == "const": cst = to_mont(cur.node[1]).tobytes()
            elif op in ("adv", "fix", "inst"): a, b = cur.node[1], cur.node[2] & 0xffffffff
            elif op == "chal": a = cur.node[1]
            elif op == "neg": a = ids[id(cur.node[1])]
            else: a, b = ids[id(cur.node[1])], ids[id(cur.node[2])]
            nodes.append(struct.pack("<4I", _OPS[op], a, b, 0) + cst)
            ids[id(cur)] = len(nodes) - 1
            stack.pop()
        return ids[id(e)]

    gates = [visit(g) for g in cs.gates]
    lookups = [([[visit(e) for e in t] for t in ins], [visit(e) for e in tab]) for ins, tab in cs.lookups]
    out = bytearray(struct.pack("<7I", 0x53435a45, 2, cs.k, cs.n_advice, cs.n_fixed, cs.n_instance, cs.n_challenges))
    out += struct.pack("<%dI" % cs.n_advice, *cs.advice_phase)
    out += struct.pack("<3I%dI" % len(cs.unblinded), cs.blinding, cs.minimum_degree or 0, len(cs.unblinded), *cs.unblinded)
    out += struct.pack("<I", cs.n_selectors)
    out += struct.pack("<I", len(nodes)) + b"".join(nodes)
    out += struct.pack("<I%dI" % len(gates), len(gates), *gates)
    out += struct.pack("<I", len(cs.perm))
    for kind, col in cs.perm:
        out += struct.pack("<2I", _KINDS[kind], col)
    out += struct.pack("<I", len(lookups))
    for ins, tab in lookups:
        out += struct.pack("<I", len(ins))
        for t in ins + [tab]:
            out += struct.pack("<I%dI" % len(t), len(t), *t)
    out += struct.pack("<I", 1 if cs.queries_given else 0)
    if cs.queries_given:
        for q in (cs.advice_queries, cs.fixed_queries, cs.instance_queries):
            out += struct.pack("<I", len(q))
            for c, r in q:
                out += struct.pack("<2I", c, r & 0xffffffff)
    return bytes(out)


def deserialize_cs(blob):
    """the inverse of serialize_cs: EZCS blob (version 2) -> ConstraintSystem with the shared sub-expressions shared again, so that
    serialize_cs(deserialize_cs(b)) == b.  A laid-out circuit can then be stored as plain data (tools/bench_circuits.py: the blob +
    JSON, nothing a reader has to unpickle)."""
    import struct
    off = [0]

    def u32(m=1):
        v = struct.unpack_from("<%dI" % m, blob, off[0]); off[0] += 4 * m
        return v if m != 1 else v[0]

    def s32(v): return v - (1 << 32) if v >= (1 << 31) else v

    magic, version, k, n_advice, n_fixed, n_instance, n_challenges = u32(7)
    if magic != 0x53435a45 or version != 2:
        raise ValueError("not a version-2 EZCS blob")
    advice_phase = list(u32(n_advice)) if n_advice != 1 else [u32()]
    blinding, minimum_degree, nu = u32(3)
    unblinded = [u32() for _ in range(nu)]
    n_selectors = u32()
    nn = u32()
    names = {v: a for a, v in _OPS.items()}
    nodes = []
    for _ in range(nn):
        op, a, b, _pad = u32(4)
        cst = blob[off[0]:off[0] + 32]; off[0] += 32
        name = names[op]
        if name == "const": e = Expr(("const", int.from_bytes(cst, "little") * RINV % R))
        elif name in ("adv", "fix", "inst"): e = Expr((name, a, s32(b)))
        elif name == "chal": e = Expr(("chal", a))
        elif name == "neg": e = Expr(("neg", nodes[a]))
        else: e = Expr((name, nodes[a], nodes[b]))
        nodes.append(e)

    def id_list():
        m = u32()
        return [nodes[u32()] for _ in range(m)]

    gates = id_list()
    kinds = {v: a for a, v in _KINDS.items()}
    perm = []
    for _ in range(u32()):
        kind, col = u32(2)
        perm.append((kinds[kind], col))
    lookups = []
    for _ in range(u32()):
        ni = u32()
        ins = [id_list() for _ in range(ni)]
        lookups.append((ins, id_list()))
    query_order = None
    if u32():
        query_order = []
        for _ in range(3):
            m = u32()
            q = []
            for _ in range(m):
                c, r = u32(2)
                q.append((c, s32(r)))
            query_order.append(q)
    if off[0] != len(blob):
        raise ValueError("trailing bytes in the EZCS blob")
    return ConstraintSystem(k, n_advice, n_fixed, gates, perm, lookups, n_instance=n_instance, advice_phase=advice_phase, n_challenges=n_challenges,
                            query_order=query_order, blinding=blinding, minimum_degree=minimum_degree or None, unblinded=unblinded, n_selectors=n_selectors)


def vk_digest(vk):
    """keccak256(keccak256(constraint-system blob) || fixed commitments || permutation commitments) mod r: the whole circuit
    description (gates, lookups, permutation, query order) is bound into the transcript, the role of halo2's
    vk.transcript_repr (a Blake2b hash of the pinned constraint system's Debug text, not reproducible without its source)."""
    t = bytearray(keccak256(serialize_cs(vk.cs)))
    for p in list(vk.fixed_commitments) + list(vk.sigma_commitments):
        x, y = (0, 0) if p is None else p
        t += x.to_bytes(32, "big") + y.to_bytes(32, "big")
    return int.from_bytes(keccak256(bytes(t)), "big") % R


# ------------------------------------------------------------------ prover
def create_proof(pk, backend, advice_values, rng, timings=None, instances=(), strict=True):
    """advice_values: list of (n,4) Montgomery arrays (rows >= usable are overwritten with blinding randomness), or a
    callable advice_values(phase, challenges) -> {column: array} for circuits with second-phase advice.
    instances: list (one per instance column) of lists of public field elements (ints); they are hashed into the
    transcript, not committed (halo2 KZG: QUERY_INSTANCE = false).
    rng.vec(m) -> (m,4) uniformly random Montgomery residues.  Returns proof bytes (EvmTranscript layout).
    strict=False lets a witness with a lookup input outside its table through (soundness tests of the verifier only)."""
    import time as _time
    _t = [_time.perf_counter()]
    def lap(name):
        if timings is not None:
            now = _time.perf_counter(); timings[name] = timings.get(name, 0.0) + now - _t[0]; _t[0] = now
    cs = pk.cs
    n, k, u = cs.n, cs.k, cs.usable
    T = EvmTranscript()
    T.common_scalar(pk.vk.digest)
    # 0. instances: absorbed, never committed
    inst_cols = []
    for vals in instances:
        for v in vals:
            T.common_scalar(v)
        col = np.zeros((n, 4), np.uint64)
        for i, v in enumerate(vals):
            col[i] = to_mont(v)
        inst_cols.append(backend.upload(col))
    assert len(inst_cols) == cs.n_instance
    # 1. advice columns, phase by phase; the phase-0 commitments seed the user challenges
    adv_cols = [None] * cs.n_advice
    user_chal = []
    for phase in (0, 1):
        idxs = [c for c in range(cs.n_advice) if cs.advice_phase[c] == phase]
        if not idxs:
            continue
        vals = advice_values(phase, list(user_chal)) if callable(advice_values) else {c: advice_values[c] for c in idxs}
        for c in idxs:
            adv_cols[c] = backend.upload(vals[c])                    # witness column -> HBM, then blind rows [u, n) in place
            if c in cs.unblinded:                                    # Blind::default() = 1, no randomness drawn (polycommit.rs:57-61)
                backend.set_rows(adv_cols[c], u, np.tile(to_mont(1), (n - u, 1)))
            else:
                backend.set_rows(adv_cols[c], u, rng.vec(n - u))
        for p in backend.commit_lagrange([adv_cols[c] for c in idxs]):
            T.write_point(p)
        if phase == 0:
            user_chal = [T.squeeze_challenge() for _ in range(cs.n_challenges)]
    lap("advice_commit")
    def col_handle(kind, c): return adv_cols[c] if kind == "adv" else inst_cols[c] if kind == "inst" else pk.fixed_values[c]
    # 2. theta; mv-lookup multiplicities m(X)
    theta, lk = None, []
    if cs.lookups:
        theta = T.squeeze_challenge()
        for ins, tab in cs.lookups:
            comp = [compress_column(cs, backend, t, theta, col_handle, user_chal) for t in ins + [tab]]
            m, missing = backend.lookup_multiplicity(comp[:-1], comp[-1], u)
            if missing and strict:                    # the reference's mv-lookup prover errors here: such a witness has no valid proof
                raise ValueError("lookup input not in table (%d rows)" % missing)
            backend.set_rows(m, u, rng.vec(n - u))
            lk.append({"inputs": comp[:-1], "table": comp[-1], "m": m})
        for d_, p in zip(lk, backend.commit_lagrange([d_["m"] for d_ in lk])):
            T.write_point(p)
    lap("lookup_m")
    # 3. beta, gamma
    beta, gamma = T.squeeze_challenge(), T.squeeze_challenge()
    # 4. permutation grand products, chained across chunks
    zs, last = [], None
    pos = 0
    for chunk in cs.perm_chunks():
        vals = [col_handle(kd, c) for kd, c in chunk]
        sigs = pk.sigma_values[pos:pos + len(chunk)]
        z = backend.permutation_product(vals, sigs, beta, gamma, pos, last, pk.omega_col)
        last = backend.get_row(z, u)
        backend.set_rows(z, u + 1, rng.vec(n - u - 1))
        zs.append(z)
        pos += len(chunk)
    for p in backend.commit_lagrange(zs) if zs else []:
        T.write_point(p)
    lap("permutation_z")
    # 4b. mv-lookup running sums phi(X)
    for d_ in lk:
        phi = backend.lookup_grand_sum(d_["inputs"], d_["table"], d_["m"], beta)
        backend.set_rows(phi, u + 1, rng.vec(n - u - 1))
        d_["phi"] = phi
    for p in backend.commit_lagrange([d_["phi"] for d_ in lk]) if lk else []:
        T.write_point(p)
    lap("lookup_phi")
    # 5. vanishing argument: random polynomial
    rnd = backend.upload(rng.vec(n))
    T.write_point(backend.commit([rnd])[0])
    # 6. y
    y = T.squeeze_challenge()
    lap("random_poly")
    # 7. quotient
    # Column-sharded backends ("per-column NTT batches shard"): every witness-dependent column has an OWNER rank
    # (round-robin over one global numbering) which alone computes its coefficient and extended forms, evaluates it at x and adds
    # it into the SHPLONK combinations; the row-sharded sweep gets its windows of every coset through one all-to-all.
    owner_of = getattr(backend, "owner_of", None)
    gidx = {"n": 0}
    def forms(handles, with_coset=True):
        polys, cosets, owners = [], [], []
        for h in handles:
            o = -1 if owner_of is None else owner_of(gidx["n"])
            gidx["n"] += 1
            mine = owner_of is None or o == backend.rank
            p_ = backend.lagrange_to_coeff(h) if mine else None
            polys.append(p_); owners.append(o)
            cosets.append(backend.coeff_to_extended(p_, cs.ext_k) if (mine and with_coset) else None)
        return polys, cosets, owners
    adv_polys, adv_cosets, adv_own = forms(adv_cols)
    _, inst_cosets, inst_own = forms(inst_cols)
    z_polys, z_cosets, z_own = forms(zs)
    m_polys, m_cosets, m_own = forms([d_["m"] for d_ in lk])
    phi_polys, phi_cosets, phi_own = forms([d_["phi"] for d_ in lk])
    lap("intt_and_coset_ntt")
    prog, cols, chal, names = quotient_program(cs, pk, adv_cosets, z_cosets, beta, gamma, y, theta, m_cosets, phi_cosets, inst_cosets, user_chal, names=True)
    hnum = backend.zeros(1 << cs.ext_k)
    if owner_of is None:
        backend.eval_program(prog, cols, chal, hnum)
    else:
        own_by_name = {}
        for c, o in enumerate(adv_own): own_by_name[("adv", c)] = o
        for c, o in enumerate(inst_own): own_by_name[("inst", c)] = o
        for j, o in enumerate(z_own): own_by_name[("z", j)] = o
        for i, o in enumerate(m_own): own_by_name[("m", i)] = o
        for i, o in enumerate(phi_own): own_by_name[("phi", i)] = o
        backend.eval_program_sharded(prog, cols, [own_by_name.get(nm, -1) for nm in names], chal, hnum)
    lap("quotient_sweep")
    backend.divide_by_vanishing(hnum, cs.ext_k)
    hcoef = backend.extended_to_coeff(hnum, cs.ext_k)
    npieces = cs.degree - 1
    pieces = [backend.slice_copy(hcoef, i * n, n) for i in range(npieces)]
    for p in backend.commit(pieces):
        T.write_point(p)
    lap("h_split_commit")
    # 8. x
    x = T.squeeze_challenge()
    w = omega(k)
    def rot_point(r): return x * pow(w, r % n if r >= 0 else n + r, R) % R
    # 9. evaluations
    if owner_of is not None:
        # owner-evaluated: every (polynomial, point) of the witness-dependent columns is evaluated by the column's owner and the scalars
        # are all_gathered once; key-side polynomials (fixed, sigma) are resident everywhere
        wanted = [(adv_polys[c], adv_own[c], rot_point(r)) for c, r in cs.advice_queries]
        for j, zp in enumerate(z_polys):
            wanted += [(zp, z_own[j], x), (zp, z_own[j], rot_point(1))] + ([(zp, z_own[j], rot_point(u))] if j + 1 < len(z_polys) else [])
        for i in range(len(lk)):
            wanted += [(phi_polys[i], phi_own[i], x), (phi_polys[i], phi_own[i], rot_point(1)), (m_polys[i], m_own[i], x)]
        shared = iter(backend.eval_by_owner(wanted, n))
        real_eval = backend.eval_poly
        def eval_poly(h, n_, pt, offset=0):
            return next(shared) if h is None or getattr(h, "_shared_eval", False) else real_eval(h, n_, pt, offset)
        for lst in (adv_polys, z_polys, m_polys, phi_polys):      # owned columns also take the gathered value: same order on all ranks
            for i_, h in enumerate(lst):
                if h is not None:
                    lst[i_] = _SharedEval(h)
    else:
        eval_poly = backend.eval_poly
    evals = {}
    for c, r in cs.advice_queries:
        evals[("adv", c, r)] = eval_poly(adv_polys[c], n, rot_point(r)); T.write_scalar(evals[("adv", c, r)])
    for c, r in cs.fixed_queries:
        evals[("fix", c, r)] = backend.eval_poly(pk.fixed_polys[c], n, rot_point(r)); T.write_scalar(evals[("fix", c, r)])
    random_eval = backend.eval_poly(rnd, n, x); T.write_scalar(random_eval)
    sigma_evals = [backend.eval_poly(h, n, x) for h in pk.sigma_polys]
    for e in sigma_evals: T.write_scalar(e)
    z_evals = []
    for j, zp in enumerate(z_polys):
        e0, e1 = eval_poly(zp, n, x), eval_poly(zp, n, rot_point(1))
        T.write_scalar(e0); T.write_scalar(e1)
        e2 = None
        if j + 1 < len(z_polys):
            e2 = eval_poly(zp, n, rot_point(u)); T.write_scalar(e2)
        z_evals.append((e0, e1, e2))
    lk_evals = []
    for mp, pp in zip(m_polys, phi_polys):
        # mv_lookup::prover::Committed::evaluate writes phi(x), phi(wx), m(x)
        e = (eval_poly(pp, n, x), eval_poly(pp, n, rot_point(1)), eval_poly(mp, n, x))
        for v_ in e: T.write_scalar(v_)
        lk_evals.append(e)
    if owner_of is not None:                          # back to plain handles (None where this rank does not own the column)
        for lst in (adv_polys, z_polys, m_polys, phi_polys):
            for i_, h in enumerate(lst):
                if isinstance(h, _SharedEval):
                    lst[i_] = h.h
    lap("evaluations")
    # 10. multiopen (SHPLONK)
    xn = pow(x, n, R)
    hcomb = backend.zeros(n)
    for i in reversed(range(npieces)):
        backend.scale(hcomb, xn, n)
        backend.axpy(hcomb, 1, pieces[i], n)
    h_eval = backend.eval_poly(hcomb, n, x)
    def rep(h, i):    # a polynomial resident on every rank counts on ONE rank in the column-sharded SHPLONK partial sums
        return h if owner_of is None or i % backend.world == backend.rank else None
    # (key, poly handle, point, eval) in halo2's query order -- advice, permutation products, lookups, fixed, sigma, h, random
    # (plonk/prover.rs step "queries"; plonk/verifier.rs builds the same chain) -- which fixes the order of SHPLONK's rotation sets
    # (first appearance) and of the commitments inside each set.  Pinned on the reference's generated EVM verifier
    # (tests/test_evm_verifier.py): set {x} = advice, m, fixed, sigma, h, random.
    qs = []
    for c, r in cs.advice_queries: qs.append((("adv", c), adv_polys[c], rot_point(r), evals[("adv", c, r)]))
    for j, zp in enumerate(z_polys):
        qs.append((("z", j), zp, x, z_evals[j][0])); qs.append((("z", j), zp, rot_point(1), z_evals[j][1]))
        if z_evals[j][2] is not None: qs.append((("z", j), zp, rot_point(u), z_evals[j][2]))
    for i, (mp, pp) in enumerate(zip(m_polys, phi_polys)):
        qs.append((("phi", i), pp, x, lk_evals[i][0])); qs.append((("phi", i), pp, rot_point(1), lk_evals[i][1]))
        qs.append((("m", i), mp, x, lk_evals[i][2]))
    for c, r in cs.fixed_queries: qs.append((("fix", c), rep(pk.fixed_polys[c], c), rot_point(r), evals[("fix", c, r)]))
    for i, (h, e) in enumerate(zip(pk.sigma_polys, sigma_evals)): qs.append((("sigma", i), rep(h, i), x, e))
    qs.append((("h",), rep(hcomb, 0), x, h_eval))
    qs.append((("rnd",), rep(rnd, 1), x, random_eval))
    shplonk_prove(backend, T, qs, n)
    lap("shplonk")
    return bytes(T.proof)


def compress_exprs(prog, tuple_exprs, theta_src, col_index, memo):
    """theta-compression of a tuple of expressions: ((e0*theta + e1)*theta + e2)... (halo2 compress_expressions)"""
    acc = lower(tuple_exprs[0], prog, col_index, memo)
    for e in tuple_exprs[1:]:
        acc = prog.calc("add", prog.calc("mul", acc, theta_src), lower(e, prog, col_index, memo))
    return acc


def compress_column(cs, backend, tuple_exprs, theta, col_handle, user_chal=()):
    """the theta-compressed lookup column over the n rows of the Lagrange domain (a gate program with ext_k = k)"""
    prog = _b.GraphProgram(cs.k, cs.k)
    cols, index = [], {}
    def col_index(kind, c):
        if kind == "chal":
            return prog.challenge(1 + c)
        if (kind, c) not in index:
            index[(kind, c)] = len(cols); cols.append(col_handle(kind, c))
        return index[(kind, c)]
    r = compress_exprs(prog, tuple_exprs, prog.challenge(0), col_index, {})
    if r[0] != _b.INTERMEDIATE:                       # a bare column / constant: materialise it
        r = prog.calc("store", r)
    out = backend.zeros(cs.n)
    backend.eval_program(prog, cols, [theta] + list(user_chal), out)
    return out


def quotient_program(cs, pk, adv_cosets, z_cosets, beta, gamma, y, theta=None, m_cosets=(), phi_cosets=(), inst_cosets=(), user_chal=(), names=False):
    """the numerator of h(X) as ONE straight-line program over the extended-coset columns: custom gates, then the
    permutation constraints, folded with y (value = value*y + constraint), as evaluate_h does"""
    prog = _b.GraphProgram(cs.k, cs.ext_k)
    cols, index, slot_names = [], {}, []
    def slot(name, handle):
        if name not in index:
            index[name] = len(cols); cols.append(handle); slot_names.append(name)
        return index[name]
    chal = [y, beta, gamma] + list(user_chal)
    def col_index(kind, c):
        if kind == "chal":
            return prog.challenge(3 + c)
        return slot((kind, c), adv_cosets[c] if kind == "adv" else inst_cosets[c] if kind == "inst" else pk.fixed_cosets[c])
    Y, BETA, GAMMA = prog.challenge(0), prog.challenge(1), prog.challenge(2)
    terms, memo = [], {}
    for g in cs.gates:
        terms.append(lower(g, prog, col_index, memo))
    if cs.perm:
        l0 = prog.column(slot("l0", pk.l0)); llast = prog.column(slot("l_last", pk.l_last)); lact = prog.column(slot("l_active", pk.l_active))
        X = prog.column(slot("X", pk.x_coset))
        one = prog.constant(to_mont(1))
        nz = len(z_cosets)
        zc = [slot(("z", j), z_cosets[j]) for j in range(nz)]
        terms.append(prog.calc("mul", l0, prog.calc("sub", one, prog.column(zc[0]))))
        zl = prog.column(zc[nz - 1])
        terms.append(prog.calc("mul", llast, prog.calc("sub", prog.calc("square", zl), zl)))
        for j in range(1, nz):
            terms.append(prog.calc("mul", l0, prog.calc("sub", prog.column(zc[j]), prog.column(zc[j - 1], cs.usable))))
        pos = 0
        for j, chunk in enumerate(cs.perm_chunks()):
            left, right = prog.column(zc[j], 1), prog.column(zc[j])
            for i, (kd, c) in enumerate(chunk):
                v = prog.column(col_index(kd, c))
                sg = prog.column(slot(("sigma", pos + i), pk.sigma_cosets[pos + i]))
                left = prog.calc("mul", left, prog.calc("add", prog.calc("add", v, prog.calc("mul", BETA, sg)), GAMMA))
                chal.append(beta * pow(DELTA, pos + i, R) % R)
                bd = prog.challenge(len(chal) - 1)
                right = prog.calc("mul", right, prog.calc("add", prog.calc("add", v, prog.calc("mul", bd, X)), GAMMA))
            terms.append(prog.calc("mul", lact, prog.calc("sub", left, right)))
            pos += len(chunk)
    if cs.lookups:
        l0 = prog.column(slot("l0", pk.l0)); llast = prog.column(slot("l_last", pk.l_last)); lact = prog.column(slot("l_active", pk.l_active))
        chal.append(theta)
        THETA = prog.challenge(len(chal) - 1)
        for i, (ins, tab) in enumerate(cs.lookups):
            phi_s, m_s = slot(("phi", i), phi_cosets[i]), slot(("m", i), m_cosets[i])
            phi, phi_next, mcol = prog.column(phi_s), prog.column(phi_s, 1), prog.column(m_s)
            fb = [prog.calc("add", compress_exprs(prog, t, THETA, col_index, memo), BETA) for t in ins]
            tb = prog.calc("add", compress_exprs(prog, tab, THETA, col_index, memo), BETA)
            prodf = fb[0]
            for f in fb[1:]:
                prodf = prog.calc("mul", prodf, f)
            ssum = None                                           # sum_j prod_{i != j} (f_i + beta)
            for j in range(len(fb)):
                pj = None
                for i2, f in enumerate(fb):
                    if i2 != j:
                        pj = f if pj is None else prog.calc("mul", pj, f)
                pj = prog.constant(to_mont(1)) if pj is None else pj
                ssum = pj if ssum is None else prog.calc("add", ssum, pj)
            lhs = prog.calc("mul", prog.calc("mul", prog.calc("sub", phi_next, phi), prodf), tb)
            rhs = prog.calc("sub", prog.calc("mul", ssum, tb), prog.calc("mul", mcol, prodf))
            terms.append(prog.calc("mul", l0, phi))
            terms.append(prog.calc("mul", llast, phi))
            terms.append(prog.calc("mul", lact, prog.calc("sub", lhs, rhs)))
    prog.horner(prog.previous(), terms, Y)
    if names:
        return prog, cols, chal, slot_names
    return prog, cols, chal


# ------------------------------------------------------------------ SHPLONK (BDFG20) multi-point opening
def group_queries(qs):
    """group (key, poly, point, eval) by polynomial key, then polynomials by their point set
    -> [(points tuple, [(poly, {pt: eval})])] in order of first appearance"""
    by_poly, order = {}, []
    for kp, p, z, e in qs:
        if kp not in by_poly:
            by_poly[kp] = (p, {}); order.append(kp)
        by_poly[kp][1][z] = e
    sets, sorder = {}, []
    for kp in order:
        p, ev = by_poly[kp]
        pts = tuple(sorted(ev))
        if pts not in sets:
            sets[pts] = []; sorder.append(pts)
        sets[pts].append((p, ev))
    return [(pts, sets[pts]) for pts in sorder]


def interpolate(points, values):
    """coefficients (low first) of the polynomial of degree < len(points) through (points, values)"""
    m = len(points)
    coeffs = [0] * m
    for i in range(m):
        num, den = [1], 1
        for j in range(m):
            if j == i: continue
            num = [(a - points[j] * b) % R for a, b in zip([0] + num, num + [0])]
            den = den * (points[i] - points[j]) % R
        s = values[i] * pow(den, -1, R) % R
        for t in range(len(num)):
            coeffs[t] = (coeffs[t] + s * num[t]) % R
    return coeffs


def eval_small(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def shplonk_prove(backend, T, qs, n):
    groups = group_queries(qs)
    ys = T.squeeze_challenge()
    all_pts = sorted({z for pts, _ in groups for z in pts})
    combos = []
    for pts, polys in groups:
        q = backend.zeros(n)
        evs = {z: 0 for z in pts}
        pw = 1
        for p, ev in polys:
            if p is not None:                          # column-sharded: only the owner adds its polynomial ...
                backend.axpy(q, pw, p, n)
            for z in pts:
                evs[z] = (evs[z] + pw * ev[z]) % R
            pw = pw * ys % R
        if getattr(backend, "owner_of", None) is not None:
            q = backend.sum_over_ranks(q, n)           # ... and the partial combinations are summed over the ranks
        r = interpolate(list(pts), [evs[z] for z in pts])
        combos.append((pts, q, r))
    v = T.squeeze_challenge()
    h = backend.zeros(n)
    pw = 1
    quot = []
    for pts, q, r in combos:
        t = backend.clone(q)
        backend.sub_low(t, r)
        for z in pts:
            backend.kate_div(t, z, n)
        backend.axpy(h, pw, t, n)
        quot.append(t)
        pw = pw * v % R
    T.write_point(backend.commit([h])[0])
    u = T.squeeze_challenge()
    zt_u = 1
    for z in all_pts:
        zt_u = zt_u * (u - z) % R
    L = backend.zeros(n)
    pw = 1
    const_term = 0
    norm = None                                        # halo2 normalises by the first set's coefficient: 1 / Z_{T \ S_0}(u)
    for pts, q, r in combos:
        zdiff = 1
        for z in all_pts:
            if z not in pts:
                zdiff = zdiff * (u - z) % R
        if norm is None:
            norm = pow(zdiff, -1, R)
        cf = pw * zdiff % R * norm % R
        backend.axpy(L, cf, q, n)
        const_term = (const_term + cf * eval_small(r, u)) % R
        pw = pw * v % R
    backend.sub_low(L, [const_term])
    backend.axpy(L, (-zt_u * norm) % R, h, n)           # Z_T(u) / Z_{T \ S_0}(u) = Z_{S_0}(u)
    backend.kate_div(L, u, n)
    T.write_point(backend.commit([L])[0])
