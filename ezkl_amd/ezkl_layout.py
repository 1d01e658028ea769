"""Witness layout (halo2 `synthesize`) for the ezkl circuits this repo proves end to end: which cell holds what, which selector is
on at which row, which cells are copy-constrained.  It follows the reference's region logic for the ops it covers so that the
constraint system produced by ezkl_circuit.py is exercised the way ezkl exercises it (every gate kind used at its real rotation,
second-phase columns filled from post-commitment challenges, constants through the fixed column), without re-implementing
ezkl's 6.8k-line layouts.rs (stays in Rust).

Covered:
  * `EinsumMatmulCircuit` = the reference's criterion bench circuit, /root/reference/benches/accum_einsum_matmul.rs:32-118
    ("ij,jk->ik", configure_einsums with one inner column + two constant cells), laid out by `Einsums::assign_einsum`
    (src/circuit/ops/chip/einsum/mod.rs:96-309): Freivalds' argument -- the output is squashed by random linear combinations
    along its axes (assign_output :311-356, RLCConfig::assign_rlc :785-866), the inputs are reduced in the order of
    reduction_planner.rs:87-205 (RLC "ij,i->j", RLC "jk,k->j", contraction "j,j->" = einsum/layouts.rs:234-318 `dot`), the
    remaining scalar goes through `prod` (:154-231) and is copy-constrained to the squashed output.
One linear coordinate (`einsum_col_coord`) is shared by the six einsum VarTensors; every op occupies the same rows in the
columns it touches.  Column overflow into a second block (assign_einsum_with_duplication) is not needed at the bench sizes and is
refused loudly.
"""
import math

import numpy as np

from . import ezkl_circuit as EC
from . import plonk as P
from .halo2_cs import ConstraintSystem

R = P.R


def signed(v):
    """a canonical field element as the signed integer it stands for"""
    return v if v < R // 2 else v - R


DIV_ERROR = "rebase dividend outside the exact-division range"
GATHER_ERROR = "gather index outside the table"
SORT_ERROR = "sort key beyond 62 bits"
SORT_MODES = ("unsorted", "smallest_index_first", "largest_index_first")       # layouts.rs:1124-1131 SortCollisionMode
RECIP_ERROR = "reciprocal operand beyond 62 bits"
SQRT_ERROR = "square-root operand outside the exact range"
ARGEXT_ERROR = "arg-extremum key beyond 62 bits"
SCATTER_ERROR = "scatter index outside the tensor"
ONEHOT_ERROR = "one-hot index outside the classes"


def clamped(s, lo, hi):
    """the signed value s held to [lo, hi] (a recording region's symbol answers for itself: a CLAMP record)"""
    return s.clamped(lo, hi) if hasattr(s, "clamped") else min(max(s, lo), hi)


def round_div(s, d):
    """the signed integer s over the constant d >= 1, rounded half away from zero: `((a as f64) / denom).round()` of const_div
    (/root/reference/src/tensor/ops.rs:2326-2331) as exact integer arithmetic, q = sgn(s) * ((|s| + d // 2) // d).  The two agree for
    |s| < 2^52 and d < 2^32: |s| and d are exact in f64, the f64 quotient is off by less than 1 / (2d) -- the least distance of s / d from
    a half that is not one -- and an exact half is representable.  Beyond 2^52 the dividend is refused."""
    mag = abs(s)
    assert mag < 1 << 52, DIV_ERROR
    return ((s > 0) - (s < 0)) * ((mag + d // 2) // d)


def recip_claim(s, S, zero_inverse):
    """the reciprocal the prover claims in `recip` for the signed input s at S = input_scale * output_scale: `zero_inverse` for s = 0, else
    the smallest integer minimiser of |y * s - S| -- the one value the gates of `optimum_convex_function` accept (f(y) <= f(y + 1) and
    f(y) < f(y - 1)) -- in exact integers: s > 0: ceil((2S - s) / (2s)); s < 0: -floor((2S + |s|) / (2|s|)).  The reference computes
    `(out_scale * (1 / (s / in_scale))).round()` in f64 (/root/reference/src/tensor/ops.rs:2353-2370): the same value except at an exact tie with
    s > 0 (s divides 2S but not S), where the f64 rounds up to y + 1 and the reference's own `less(f(y + 1), f(y))` refuses it.  (A
    recording region's symbol answers for itself: a RECIP record.)"""
    if hasattr(s, "recip_claim"):
        return s.recip_claim(S, zero_inverse)
    assert abs(s) < 1 << 62, RECIP_ERROR
    if s == 0:
        return zero_inverse
    if s > 0:
        return -((s - 2 * S) // (2 * s))
    return -((2 * S - s) // (-2 * s))


def sqrt_claim(s, scale):
    """the root the prover claims in `sqrt` for the signed input s: with T = s * scale, 0 for T <= 0, else the integer nearest to sqrt(T)
    (a tie would need T = r^2 + r + 1/4) -- `(scale * (s / scale).sqrt()).round()` of /root/reference/src/tensor/ops.rs:1844-1852 in exact
    integers, and the one value the gates accept.  (A recording region's symbol answers for itself: an ISQRT record.)"""
    if hasattr(s, "sqrt_claim"):
        return s.sqrt_claim(scale)
    T = s * scale
    assert abs(s) < 1 << 62 and T < 1 << 62, SQRT_ERROR
    if T <= 0:
        return 0
    r = math.isqrt(T)
    return r + (T - r * r > r)


def zero_recip(output_scale, eps):
    """`zero_recip` (/root/reference/src/tensor/ops.rs:2385-2395): (out_scale * (1 / (0 + eps))).round(), the constant `recip` gives a zero input"""
    v = float(output_scale) * (1.0 / (0.0 + eps))
    return int(math.copysign(math.floor(abs(v) + 0.5), v))


class Region:
    """cells, selector activations and copy constraints of one synthesis pass"""

    def __init__(self, cs, k):
        self.cs, self.k, self.n = cs, k, 1 << k
        self.usable = self.n - cs.blinding_factors() - 1
        self.advice = {}                               # advice column index -> list of n ints
        self.fixed = {}
        self.activations = [None] * len(cs.selectors)   # per selector: numpy bool rows, allocated on first use
        self.copies = []                               # ((kind, col, row), (kind, col, row))
        self.coord = 0                                 # einsum_col_coord
        self.const_cells = {}                          # value -> (fixed col, row)
        self.const_next = 0

    def column(self, col):
        store = self.advice if col.kind == "adv" else self.fixed
        if col.index not in store:
            store[col.index] = [0] * self.n
        return store[col.index]

    def put_cell(self, col, row, v):
        """the value of one cell; answers what later ops read of it (the value itself: a recording region answers the cell's symbol)"""
        self.column(col)[row] = v
        return v

    def enable(self, selector, row):
        assert row < self.usable
        a = self.activations[selector.index]
        if a is None:
            a = self.activations[selector.index] = np.zeros(self.n, bool)
        a[row] = True

    def copy(self, a, b):
        if a != b:
            self.copies.append((a, b))

    def constant(self, const_cols, value):
        """a cell of the constant fixed column holding `value` (assign_constant: one cell per distinct value)"""
        value %= R
        if value not in self.const_cells:
            col = const_cols[self.const_next // self.usable]
            row = self.const_next % self.usable
            self.const_next += 1
            self.column(col)[row] = value
            self.const_cells[value] = ("fix", col.index, row)
        return self.const_cells[value]

    def selector_rows(self, dense=True):
        """one boolean row-vector per selector (None for a selector that is never on, unless dense)"""
        return [np.zeros(self.n, bool) if (a is None and dense) else a for a in self.activations]


class Val:
    """a value with the cell it was last assigned to (ValType::PrevAssigned) or the constant it is (ValType::Constant)"""
    __slots__ = ("v", "cell", "const")

    def __init__(self, v, cell=None, const=False):
        self.v, self.cell, self.const = v % R, cell, const


class EinsumMatmulCircuit:
    """benches/accum_einsum_matmul.rs MyCircuit for "ij,jk->ik" with square len x len inputs"""
    plan_domain, plan_tables = b"phased:", False       # (what witness_plan asks of a class: see LayoutCircuit)

    def __init__(self, k, length, num_inner_cols=1):
        self.k, self.len, self.w = k, length, num_inner_cols
        dims = {"i": length, "j": length, "k": length}
        # analyze_single_equation (einsum/analysis.rs:74-209) for this equation
        out_red = length * length + length                 # RLC over k for every i, then over i
        in_red = 2 * length * length + length              # RLC ij,i->j ; RLC jk,k->j ; dot j,j->
        self.reduction_length = out_red + in_red
        cs = self.cs = ConstraintSystem()
        self.base = type("Cfg", (), {})()
        self.einsums = EC.Einsums(cs, self.reduction_length, 2, num_inner_cols, k)
        self.const_cols = EC.VarTensor.constant_cols(cs, k, 2)
        cs.chunk_lookups()
        assert all(v.num_blocks() == 1 for v in self.einsums.inputs + self.einsums.outputs), "column overflow (duplication) is not laid out here"
        assert num_inner_cols == 1, "one inner column, as in the reference bench"
        self.standalone = True                             # the columns are this circuit's own: a witness plan can be recorded

    @property
    def n_inputs(self):
        """the entries of A, then of B, row-major: the input vector of a witness plan"""
        return 2 * self.len * self.len

    @classmethod
    def over(cls, gc, length):
        """the same layout over the Freivalds columns of an existing GraphConfig (BaseConfig::configure_einsums), written into the
        caller's region next to its other ops (TransformerSurrogateCircuit)"""
        self = cls.__new__(cls)
        self.k, self.len, self.w = gc.settings.logrows, length, 1
        self.cs, self.einsums, self.const_cols = gc.cs, gc.base.einsums, gc.const_cols
        self.reduction_length = 3 * length * length + 2 * length
        assert all(v.num_blocks() == 1 and v.num_inner_cols == 1 for v in self.einsums.inputs + self.einsums.outputs)
        return self

    # ---- the pieces of assign_einsum -------------------------------------------------------------------------------
    def _assign(self, region, var, vals, live):
        """region.assign_einsum: vals (list of Val) go to rows coord.. of `var`; a previously assigned value is copy-constrained,
        a constant is copy-constrained to the fixed column.  `live`: fill values (False in the phase that does not own the column)."""
        col = var.inner[0][0]
        out = []
        for t, val in enumerate(vals):
            row = region.coord + t
            assert row < region.usable, "einsum column overflow"
            v = region.put_cell(col, row, val.v) if live else val.v
            cell = ("adv", col.index, row)
            if val.const:
                region.copy(cell, region.constant(self.const_cols, val.v))
            elif val.cell is not None:
                region.copy(cell, val.cell)
            out.append(Val(v, cell))
        return out

    def _rlc(self, region, gate_idx, vals, rlc, rlc_len, phase, cur_phase):
        """RLCConfig::assign_rlc with block width 1: out[0] = c*v0 (init), out[t] = out[t-1]*c + c*v[t] (acc), c = challenge `gate_idx`;
        the running values are `rlc`'s (see `sequence`)"""
        g = self.einsums.rlc[gate_idx]
        in_var = [self.einsums.inputs[0], self.einsums.inputs[2]][phase]
        out_var = self.einsums.outputs[1]
        results = []
        for s in range(0, len(vals), rlc_len):
            chunk = self._assign(region, in_var, vals[s:s + rlc_len], live=(phase == 0 or cur_phase == 1))
            outs = self._assign(region, out_var, rlc(chunk, gate_idx), live=(cur_phase == 1))
            init_s, acc_s = g["selectors"][(phase, 0)]
            region.enable(init_s, region.coord)
            for t in range(1, len(chunk)):
                region.enable(acc_s, region.coord + t)
            results.append(outs[-1])
            region.coord += len(chunk)
        return results

    def sequence(self, region, A, B, O, rlc, dot, cur):
        """assign_einsum for "ij,jk->ik", stated once: `synthesize` runs it on integers, the witness-plan recorder (witness_plan.py) on
        symbols.  A, B: len x len Vals; O: the len * len Vals of the product, row-major; rlc(vals, challenge index) and dot(xs, ys)
        answer the running values of a random linear combination / of a dot product over assigned Vals; cur: the phase being
        synthesized (0: first-phase columns, selectors, copies; 1: everything)."""
        L = self.len
        E = self.einsums
        # assign_output: RLC along k (challenge 1, first-phase input), then along i (challenge 0, second-phase input)
        inter = self._rlc(region, 1, O, rlc, L, 0, cur)
        inter = self._rlc(region, 0, inter, rlc, L, 1, cur)
        squashed_out = self._assign(region, E.outputs[1], inter, live=(cur == 1))[0]
        region.coord += 1
        # input reductions (reduction_planner::input_reductions("ij,jk->ik")): axis i, axis k, then the common axis j
        colsA = [A[i][j] for j in range(L) for i in range(L)]          # for every j: the slice A[:, j]
        ra = self._rlc(region, 0, colsA, rlc, L, 0, cur)
        rowsB = [B[j][kk] for j in range(L) for kk in range(L)]        # for every j: the slice B[j, :]
        rb = self._rlc(region, 1, rowsB, rlc, L, 0, cur)
        # contraction "j,j->": dot of two second-phase vectors (einsum/layouts.rs `dot`, BothSecondPhase)
        sel = E.contraction_selectors
        xa = self._assign(region, E.inputs[2], ra, live=(cur == 1))
        xb = self._assign(region, E.inputs[3], rb, live=(cur == 1))
        outs = self._assign(region, E.outputs[1], dot(xa, xb), live=(cur == 1))
        region.enable(sel[((EC.DOTINIT, EC.BOTH_SECOND), 0, 0)], region.coord)
        for t in range(1, L):
            region.enable(sel[((EC.DOT, EC.BOTH_SECOND), 0, 0)], region.coord + t)
        region.coord += L
        # prod over the remaining scalars (one), second phase: CUMPRODINIT
        self._assign(region, E.inputs[2], [outs[-1]], live=(cur == 1))
        squashed_in = self._assign(region, E.outputs[1], [Val(outs[-1].v)], live=(cur == 1))[0]
        region.enable(sel[((EC.CUMPRODINIT, EC.SECOND_PHASE), 0, 0)], region.coord)
        region.coord += 1
        region.copy(squashed_in.cell, squashed_out.cell)
        return region

    def synthesize(self, a, b, challenges=None, region=None):
        """a, b: len x len integer arrays (values mod r).  challenges=None: first phase (first-phase columns, selectors, copies);
        else the two challenges: everything.  Returns the Region (a fresh one unless the caller hands its own)."""
        L = self.len
        if region is None:
            region = Region(self.cs, self.k)
        A = [[Val(int(a[i][j])) for j in range(L)] for i in range(L)]
        B = [[Val(int(b[j][kk])) for kk in range(L)] for j in range(L)]
        return self.sequence(region, A, B, *self.host_ops(a, b, challenges))

    def host_ops(self, a, b, challenges=None):
        """what `sequence` takes besides the operands when it runs on integers: (the product's Vals, rlc, dot, the phase being synthesized)"""
        cur = 0 if challenges is None else 1
        O = [Val(int(v)) for v in self.matmul(a, b).reshape(-1)]
        def rlc(vals, ci):
            if cur == 0:
                return [Val(0)] * len(vals)
            c, acc, run = challenges[ci], 0, []
            for v in vals:
                acc = (acc * c + c * v.v) % R
                run.append(Val(acc))
            return run
        def dot(xs, ys):
            acc, run = 0, []
            for x, y in zip(xs, ys):
                acc = (acc + x.v * y.v) % R
                run.append(Val(acc))
            return run
        return O, rlc, dot, cur

    def plan_identity(self):
        """what a witness plan of this circuit depends on (witness_plan.params_hash)"""
        return ("%s:k=%d:len=%d:ij,jk->ik" % (type(self).__name__, self.k, self.len)).encode()

    @staticmethod
    def matmul(a, b):
        """the einsum output the prover witnesses: exact integer product of quantised (small) inputs"""
        a64, b64 = np.asarray(a, np.int64), np.asarray(b, np.int64)
        bound = int(np.abs(a64).max(initial=0)) * int(np.abs(b64).max(initial=0)) * a64.shape[1]
        assert bound < 1 << 62, "inputs too large for the exact int64 product"
        return a64 @ b64

    # ---- what keygen / the prover need ------------------------------------------------------------------------------
    def keygen_inputs(self, a, b):
        """-> (plonk.ConstraintSystem, fixed columns (ints), copies over cs.perm positions, rows used)"""
        region = self.synthesize(a, b)
        n = 1 << self.k
        sel_cols = self.cs.compress_selectors(region.selector_rows(dense=False))
        if n <= 1 << 12:                               # small circuits: plain ints (MockProver); large: numpy (ints_to_limbs is vectorised)
            sel_cols = [c.tolist() for c in sel_cols]
        cs = self.cs.to_plonk(self.k)
        n_pre = cs.n_fixed - len(sel_cols)
        fixed = [region.fixed.get(c, [0] * n) for c in range(n_pre)] + list(sel_cols)
        pos = {kc: i for i, kc in enumerate(cs.perm)}
        copies = [((pos[(x[0], x[1])], x[2]), (pos[(y[0], y[1])], y[2])) for x, y in region.copies]
        return cs, fixed, copies, region.coord

    def advice_fn(self, a, b, n_advice):
        """the per-phase witness callback of create_proof: phase 0 -> first-phase columns, phase 1 (with the challenges) -> the
        second-phase columns"""
        n = 1 << self.k
        def fn(phase, challenges):
            region = self.synthesize(a, b, None if phase == 0 else tuple(challenges[:2]))
            return {c.index: region.advice.get(c.index, [0] * n) for c in self.cs.advice if c.phase == phase}
        return fn


EINSUM_OPERANDS_ERROR = "the einsum layout takes two operands"
EINSUM_BASE_OPS_ERROR = "an einsum the reference lays out with base ops, not with Freivalds' argument"
EINSUM_REPEAT_ERROR = "an einsum operand with a repeated axis"
EINSUM_OVERFLOW_ERROR = "column overflow (duplication) is not laid out here"
EINSUM_WIDTH_ERROR = "one inner column, as in the reference bench"
EINSUM_SHAPE_ERROR = "an einsum operand of another size than its axes give"


class _HostEinsumOps:
    """the running values `EinsumCircuit.sequence` asks for, on integers: cur = 0 answers zeros for whatever a challenge enters (those
    cells are not written in the first phase)"""

    def __init__(self, challenges):
        self.challenges, self.cur = challenges, 0 if challenges is None else 1

    def rlc(self, vals, ci):
        if self.cur == 0:
            return [Val(0)] * len(vals)
        c, acc, run = self.challenges[ci], 0, []
        for v in vals:
            acc = (acc * c + c * v.v) % R
            run.append(Val(acc))
        return run

    def dot(self, xs, ys):
        acc, run = 0, []
        for x, y in zip(xs, ys):
            acc = (acc + x.v * y.v) % R
            run.append(Val(acc))
        return run

    def sum(self, xs):
        acc, run = 0, []
        for x in xs:
            acc = (acc + x.v) % R
            run.append(Val(acc))
        return run

    def prod(self, xs):
        acc, run = 1, []
        for x in xs:
            acc = acc * x.v % R
            run.append(Val(acc))
        return run

    def mul(self, xs, ys):
        return [Val(x.v * y.v) for x, y in zip(xs, ys)]


class EinsumCircuit(EinsumMatmulCircuit):
    """`Einsums::assign_einsum` (/root/reference/src/circuit/ops/chip/einsum/mod.rs:105-300) for any two-operand equation the reference
    lays out with Freivalds' argument, at block width 1 in one block: the plan is einsum_plan's (reduction_planner.rs, analysis.rs), the
    output is squashed by `assign_output` (:302-348), the operands by the plan's reductions -- an RLC (RLCConfig::assign_rlc :785-866), a
    pairwise product (`assign_pairwise_mult` :351-376, einsum/layouts.rs:16-93 `pairwise`) or a contraction (`assign_input_contraction`
    :378-420: `sum` layouts.rs:95-163 of one tensor, `dot` :233-315 of two) --, the scalars that remain go through `prod` (:165-231) and
    the result is copy-constrained to the squashed output.  dims: axis -> extent for every axis of an operand; an operand is its entries
    row-major in the order of its own expression.  With standalone columns (this constructor) max_num_output_axes and the capacity come
    from the analysis; `over` lays the same sequence over the Freivalds columns of a GraphConfig.  Three or more operands (`multi_dot`),
    the base-op strategy and a column that overflows into a second block are refused by name."""
    plan_domain = b"einsum:"

    def __init__(self, k, equation, dims, num_inner_cols=1):
        self._plan(k, equation, dims, num_inner_cols)
        cs = self.cs = ConstraintSystem()
        self.base = type("Cfg", (), {})()
        self.einsums = EC.Einsums(cs, self.reduction_length, self.analysis.num_output_axes, num_inner_cols, k)
        self.const_cols = EC.VarTensor.constant_cols(cs, k, 2)
        cs.chunk_lookups()
        assert all(v.num_blocks() == 1 for v in self.einsums.inputs + self.einsums.outputs), EINSUM_OVERFLOW_ERROR
        self.standalone = True

    def _plan(self, k, equation, dims, num_inner_cols):
        """everything that is refused, before a column exists"""
        from . import einsum_plan as EP
        inputs_eq, _ = equation.split("->")
        exprs = inputs_eq.split(",")
        if len(exprs) != 2:
            raise ValueError(EINSUM_OPERANDS_ERROR)
        if any(len(set(e)) != len(e) for e in exprs):
            raise ValueError(EINSUM_REPEAT_ERROR)
        if num_inner_cols != 1:
            raise ValueError(EINSUM_WIDTH_ERROR)
        self.k, self.w, self.equation = k, num_inner_cols, equation
        self.dims = {c: int(dims[c]) for e in exprs for c in e}
        self.analysis = EP.einsum_analysis(equation, self.dims)
        if self.analysis.strategy != EP.FREIVALDS:
            raise ValueError(EINSUM_BASE_OPS_ERROR)
        self.reductions = EP.einsum_reductions(self.analysis.equation)
        self.reduction_length = self.analysis.reduction_length
        self.exprs = self.analysis.equation.split("->")[0].split(",")              # without the trivial axes; the entries stay in place
        self.sizes = [math.prod(self.dims[c] for c in e) for e in self.exprs]
        self.out_shape = [self.dims[c] for c in self.analysis.output_indices]

    @property
    def n_inputs(self):
        """the entries of the first operand, then of the second, row-major: the input vector of a witness plan"""
        return sum(self.sizes)

    @classmethod
    def over(cls, gc, equation, dims):
        """the same layout over the Freivalds columns of an existing GraphConfig (BaseConfig::configure_einsums), written into the
        caller's region next to its other ops (BaseRegion.einsum)"""
        self = cls.__new__(cls)
        self._plan(gc.settings.logrows, equation, dims, gc.settings.num_inner_cols)
        self.cs, self.einsums, self.const_cols = gc.cs, gc.base.einsums, gc.const_cols
        assert len(self.einsums.rlc) >= self.analysis.num_output_axes, "the configuration has fewer RLC gates than the einsum has output axes"
        assert all(v.num_blocks() == 1 and v.num_inner_cols == 1 for v in self.einsums.inputs + self.einsums.outputs), EINSUM_OVERFLOW_ERROR
        return self

    # ---- the pieces of assign_einsum -------------------------------------------------------------------------------
    def _live(self, var, cur):
        return cur == 1 or not any(var is v for v in (self.einsums.inputs[2], self.einsums.inputs[3], self.einsums.outputs[1]))

    def _vars(self, phases):
        """ContractionConfig::get_input_vars / get_output_var (mod.rs:463-481) -> (InputPhases, input VarTensors, output VarTensor)"""
        E = self.einsums
        ph = {(0,): EC.FIRST_PHASE, (1,): EC.SECOND_PHASE, (0, 0): EC.BOTH_FIRST, (0, 1): EC.MIXED, (1, 0): EC.MIXED, (1, 1): EC.BOTH_SECOND}[tuple(phases)]
        ins = {EC.FIRST_PHASE: [E.inputs[0]], EC.SECOND_PHASE: [E.inputs[2]], EC.BOTH_FIRST: [E.inputs[0], E.inputs[1]],
               EC.MIXED: [E.inputs[0], E.inputs[2]], EC.BOTH_SECOND: [E.inputs[2], E.inputs[3]]}[ph]
        return ph, ins, E.outputs[0] if ph in (EC.FIRST_PHASE, EC.BOTH_FIRST) else E.outputs[1]

    def _rlc_placed(self, region, gate_idx, vals, rlc, rlc_len, phase, cur):
        """`_rlc`, answering the placed inputs beside the results"""
        g = self.einsums.rlc[gate_idx]
        in_var, out_var = [self.einsums.inputs[0], self.einsums.inputs[2]][phase], self.einsums.outputs[1]
        results, placed = [], []
        for s in range(0, len(vals), rlc_len):
            chunk = self._assign(region, in_var, vals[s:s + rlc_len], live=(phase == 0 or cur == 1))
            outs = self._assign(region, out_var, rlc(chunk, gate_idx), live=(cur == 1))
            init_s, acc_s = g["selectors"][(phase, 0)]
            region.enable(init_s, region.coord)
            for t in range(1, len(chunk)):
                region.enable(acc_s, region.coord + t)
            results.append(outs[-1])
            placed += chunk
            region.coord += len(chunk)
        return results, placed

    def _accumulated(self, region, ins, running, ops_kind, phases, cur):
        """einsum/layouts.rs `sum` (:95-163), `prod` (:165-231) and `dot` (:233-315) at block width 1: the tensors into the input
        VarTensors of their phases, the running value beside them, the INIT selector on the first row and the accumulating one after"""
        init_op, op = ops_kind
        ph, in_vars, out_var = self._vars(phases)
        placed = [self._assign(region, var, vals, live=self._live(var, cur)) for var, vals in zip(in_vars, ins)]
        outs = self._assign(region, out_var, running(*placed), live=self._live(out_var, cur))
        sel = self.einsums.contraction_selectors
        region.enable(sel[((init_op, ph), 0, 0)], region.coord)
        for t in range(1, len(outs)):
            region.enable(sel[((op, ph), 0, 0)], region.coord + t)
        region.coord += len(outs)
        return outs[-1]

    def _pairwise_mult(self, region, ins, ops, phases, cur):
        """einsum/layouts.rs:16-93 `pairwise` with BaseOp::Mult: one MULT row per element"""
        ph, in_vars, out_var = self._vars(phases)
        placed = [self._assign(region, var, vals, live=self._live(var, cur)) for var, vals in zip(in_vars, ins)]
        outs = self._assign(region, out_var, ops.mul(*placed), live=self._live(out_var, cur))
        for t in range(len(outs)):
            region.enable(self.einsums.contraction_selectors[((EC.MULT, ph), 0, 0)], region.coord + t)
        region.coord += len(outs)
        return outs

    def sequence(self, region, operands, O, ops, cur):
        """assign_einsum, stated once: `synthesize` runs it on integers, the witness-plan recorder (witness_plan.py) on symbols.
        operands: the two operands as flat row-major lists of Vals; O: the Vals of the product, row-major over the output axes; ops:
        rlc(vals, challenge index), dot(xs, ys), sum(xs), prod(xs) -- the running values over assigned Vals -- and mul(xs, ys); cur: the
        phase being synthesized (0: first-phase columns, selectors, copies; 1: everything).  Returns the product as the Vals
        `assign_output`'s first RLC placed in the first-phase input column."""
        from . import einsum_plan as EP
        E, dims = self.einsums, self.dims
        assert [len(t) for t in operands] == self.sizes and len(O) == math.prod(self.out_shape), EINSUM_SHAPE_ERROR
        # assign_output (:302-348): the axes in reverse, phase 0 for the first RLC and phase 1 after it, then the squashed scalar
        inter, product, n_axes = list(O), None, len(self.out_shape)
        for idx in range(n_axes):
            inter, placed = self._rlc_placed(region, n_axes - 1 - idx, inter, ops.rlc, self.out_shape[n_axes - 1 - idx], 1 if idx else 0, cur)
            product = placed if product is None else product
        out_var = E.outputs[1 if n_axes else 0]
        squashed_out = self._assign(region, out_var, inter, live=self._live(out_var, cur))[0]
        region.coord += 1
        # the input reductions (:168-283)
        tensors = [(e, list(t)) for e, t in zip(self.exprs, operands)]
        reduced_phase = 0
        for red in self.reductions:
            in_exprs, out_expr = red.expression.split("->")
            in_exprs = in_exprs.split(",")
            inputs = [tensors[i] for i in EP.reduction_inputs(red)]
            flat = [[] for _ in inputs]
            for at in np.ndindex(*[dims[c] for c in out_expr]):                   # one running value per index tuple of the remaining axes
                fixed = dict(zip(out_expr, at))
                for t, (expr, vals) in enumerate(inputs):
                    ranges = [[fixed[c]] if c in fixed else range(dims[c]) for c in expr]
                    strides = self._strides([dims[c] for c in expr])
                    flat[t] += [vals[sum(i * s for i, s in zip(pos, strides))] for pos in self._product(ranges)]
            if isinstance(red, EP.RLC):
                result, _ = self._rlc_placed(region, red.challenge_index, flat[0], ops.rlc, dims[red.axis], red.input_phase, cur)
            elif red.axis is None:                                                # assign_pairwise_mult (:351-376)
                phases = list(red.input_phases)
                if phases[0] > phases[1]:
                    flat, phases = flat[::-1], phases[::-1]
                result = self._pairwise_mult(region, flat, ops, phases, cur)
            else:                                                                 # assign_input_contraction (:378-420)
                length, result = dims[red.axis], []
                for s in range(0, len(flat[0]), length):
                    chunk = [f[s:s + length] for f in flat]
                    if len(chunk) == 1:
                        result.append(chunk[0][0] if length == 1 else
                                      self._accumulated(region, chunk, ops.sum, (EC.SUMINIT, EC.SUM), red.input_phases, cur))
                    else:
                        phases = list(red.input_phases)
                        if phases[0] > phases[1]:
                            chunk, phases = chunk[::-1], phases[::-1]
                        result.append(self._accumulated(region, chunk, ops.dot, (EC.DOTINIT, EC.DOT), phases, cur))
            tensors.append((out_expr, result))
            reduced_phase = EP.reduction_output_phase(red)
        # the scalars that remain, through `prod`; the result is the squashed output
        scalars = [vals[0] for _, vals in tensors if len(vals) == 1]
        squashed_in = self._accumulated(region, [scalars], ops.prod, (EC.CUMPRODINIT, EC.CUMPROD), [reduced_phase], cur)
        region.copy(squashed_in.cell, squashed_out.cell)
        return product

    @staticmethod
    def _strides(shape):
        out, s = [], 1
        for d in reversed(shape):
            out.append(s)
            s *= d
        return out[::-1]

    @staticmethod
    def _product(ranges):
        out = [()]
        for r in ranges:
            out = [p + (i,) for p in out for i in r]
        return out

    # ---- on integers ------------------------------------------------------------------------------------------------
    def einsum(self, a, b):
        """the product the prover witnesses: the exact contraction over the integers, flat and row-major over the output axes"""
        shapes = [[self.dims[c] for c in e] for e in self.exprs]
        a, b = (np.array([int(v) for v in np.asarray(x, dtype=object).reshape(-1)], dtype=object).reshape(s) for x, s in zip((a, b), shapes))
        out = np.einsum(self.analysis.equation, a, b)
        return [int(v) for v in np.asarray(out, dtype=object).reshape(-1)]

    def host_ops(self, a, b, challenges=None):
        """what `sequence` takes besides the operands when it runs on integers: (the product's Vals, the running values, the phase)"""
        ops = _HostEinsumOps(challenges)
        return [Val(v) for v in self.einsum(a, b)], ops, ops.cur

    def synthesize(self, a, b, challenges=None, region=None):
        """a, b: the operands as integer arrays (values mod r, or signed).  challenges=None: first phase (first-phase columns, selectors,
        copies); else the challenges, one per output axis: everything.  Returns the Region (a fresh one unless the caller hands its own)."""
        if region is None:
            region = Region(self.cs, self.k)
        flat = lambda x: [Val(int(v)) for v in np.asarray(x, dtype=object).reshape(-1)]
        self.sequence(region, [flat(a), flat(b)], *self.host_ops(a, b, challenges))
        return region

    def plan_identity(self):
        dims = ",".join("%s=%d" % (c, self.dims[c]) for c in sorted(self.dims))
        return ("%s:k=%d:%s:%s" % (type(self).__name__, self.k, self.equation, dims)).encode()

    def advice_fn(self, a, b, n_advice):
        n, nc = 1 << self.k, self.analysis.num_output_axes
        def fn(phase, challenges):
            region = self.synthesize(a, b, None if phase == 0 else tuple(challenges[:nc]))
            return {c.index: region.advice.get(c.index, [0] * n) for c in self.cs.advice if c.phase == phase}
        return fn


def ints_to_mont(colv):
    """list of n canonical ints -> (n, 4) u64 Montgomery array (plain Python: small columns / tests)"""
    if isinstance(colv, np.ndarray):
        colv = colv.tolist()
    M = 1 << 256
    return np.frombuffer(b"".join((int(v) % R * M % R).to_bytes(32, "little") for v in colv), np.uint64).reshape(len(colv), 4).copy()


_R_LIMBS = np.array([(R >> (64 * i)) & 0xffffffffffffffff for i in range(4)], np.uint64)


def ints_to_limbs(colv):
    """n field elements (ints mod r, or a numpy array of small signed ints) -> (n, 4) u64 CANONICAL limbs, vectorised for what
    witness columns mostly hold: small values and negated small values (integer_rep_to_felt, src/fieldutils.rs:9-17)"""
    n = len(colv)
    out = np.zeros((n, 4), np.uint64)
    if isinstance(colv, np.ndarray) and colv.dtype != object:
        v = colv.astype(np.int64)
        small, mag = v >= 0, np.abs(v).astype(np.uint64)
        out[small, 0] = mag[small]
        neg = ~small
    else:
        arr = np.asarray(colv, dtype=object)
        small = arr < (1 << 62)
        out[small, 0] = arr[small].astype(np.uint64)
        rest = np.nonzero(~small)[0]
        negv = R - arr[rest]                               # object arithmetic: negated small values become small again
        isneg = negv < (1 << 62)
        full = rest[~isneg]
        if len(full):
            out[full] = np.frombuffer(b"".join(int(arr[i]).to_bytes(32, "little") for i in full), np.uint64).reshape(len(full), 4)
        neg = np.zeros(n, bool)
        neg[rest[isneg]] = True
        mag = np.zeros(n, np.uint64)
        mag[rest[isneg]] = negv[isneg].astype(np.uint64)
    if neg.any():                                          # r - m with m < 2^62 < r's lowest limb: no borrow leaves limb 0
        out[neg] = _R_LIMBS
        out[neg, 0] = _R_LIMBS[0] - mag[neg]
    return out


_PINNED = []                                               # page-locked buffers handed out by cols_to_mont(pinned=True): kept alive here


def cols_to_mont(cols, gpu=None, pinned=False):
    """columns of field elements -> (n, 4) u64 Montgomery arrays.  With gpu = ezkl_amd.backend the canonical limbs are multiplied
    by R^2 on the device (one Montgomery product per element); without, element by element in Python.  pinned: the arrays live in
    page-locked host memory (ezkl_hip_host_malloc), what a prover's synthesis should fill so that uploads run at PCIe speed."""
    if gpu is None:
        return [ints_to_mont(c) for c in cols]
    r2 = P.to_mont((1 << 256) % R)
    out = []
    for c in cols:
        buf = gpu.DeviceBuffer.from_numpy(ints_to_limbs(c))
        gpu.vec_scale(buf.ptr, r2, buf.ptr, len(c))
        a = buf.to_numpy(shape=(len(c), 4))
        if pinned:
            pa = gpu.PinnedArray((len(c), 4))
            pa.array[:] = a
            _PINNED.append(pa)
            a = pa.array
        else:
            a = a.copy()
        out.append(a)
    return out


# =====================================================================================================================
# Base-op layouts (src/circuit/ops/layouts.rs) over the three model VarTensors, with RegionCtx's single linear coordinate
# =====================================================================================================================
class BaseRegion(Region):
    """RegionCtx (src/circuit/ops/region.rs) for BaseConfig's columns: `assign` writes a tensor at the linear coordinate of a
    VarTensor (block, inner column, row = VarTensor::cartesian_coord), `increment` advances it; constants are assigned with a copy
    constraint to ONE cell of the constant column per distinct value (first use) and to that first advice cell afterwards
    (assigned_constants, src/tensor/var.rs assign_value); previously assigned values are copy-constrained to their cell."""

    def __init__(self, gc, witness=True):
        super().__init__(gc.cs, gc.settings.logrows)
        self.gc, self.base, self.w = gc, gc.base, gc.settings.num_inner_cols
        self.inputs, self.output = [gc.advices[0], gc.advices[1]], gc.advices[2]
        self.linear = 0
        self.witness = witness
        self.first_const = {}                          # value -> first advice cell holding it
        self.const_order = []                          # (value, advice cell) in order of first use: the floor planner's fixed cells
        self.decomp = None                             # RegionCtx's (base, legs), region.rs `base()` / `legs()`: set by the circuit's layout
        self.shuffle_index = 0                         # region.shuffle_index(): the constant that keeps the sorts of a region apart in the argument
        self.dynamic_lookup_index = 0                  # region.dynamic_lookup_index(): the same for the `select`s of a region
        # region.rs:548-559 `update_max_min_lookup_inputs`: the running extrema of the signed inputs to every static lookup, both from 0
        # (graph/mod.rs:166-167) -- a witness file's min_lookup_inputs / max_lookup_inputs
        self.min_lookup_inputs = self.max_lookup_inputs = 0

    def cell_of(self, var, linear):
        x, y, z = var.cartesian_coord(linear)
        assert x < var.num_blocks(), "circuit does not fit: raise total_assignments"
        return var.inner[x][y], z

    def put(self, var, linear, val):
        col, row = self.cell_of(var, linear)
        cell = ("adv", col.index, row)
        if self.witness:
            self.column(col)[row] = val.v
        if val.const:
            first = self.first_const.get(val.v)
            if first is None:
                self.first_const[val.v] = cell
                self.const_order.append((val.v, cell))
            else:
                self.copy(cell, first)
        elif val.cell is not None:
            self.copy(cell, val.cell)
        return Val(val.v, cell)

    def assign(self, var, vals, offset=None):
        base = self.linear if offset is None else offset
        return [self.put(var, base + t, v) for t, v in enumerate(vals)]

    def increment(self, m): self.linear += m

    def flush(self):
        rem = self.linear % self.w
        if rem:
            self.linear += self.w - rem

    def finish(self, const_cols):
        """the floor planner's constants: one fixed cell per distinct constant, in order of first use, copied to its first advice cell"""
        u = self.usable
        for i, (v, cell) in enumerate(self.const_order):
            col = const_cols[i // u]
            self.column(col)[i % u] = v
            self.copy(("fix", col.index, i % u), cell)

    # ---- layouts.rs ------------------------------------------------------------------------------------------------
    def pairwise(self, a, b, op):
        """layouts.rs:2917-2990 (both operands already broadcast to one length)"""
        assert len(a) == len(b)
        ia, ib = self.assign(self.inputs[0], a), self.assign(self.inputs[1], b)
        f = {EC.ADD: lambda x, y: x + y, EC.SUB: lambda x, y: x - y, EC.MULT: lambda x, y: x * y}[op]
        out = self.assign(self.output, [Val(f(x.v, y.v)) for x, y in zip(ia, ib)])
        for t in range(len(out)):
            x, y, z = self.inputs[0].cartesian_coord(self.linear + t)
            self.enable(self.base.selectors[(op, x, y)], z)
        self.increment(len(out))
        return out

    def enforce_equality(self, a, b):
        """layouts.rs:4959-4981"""
        ia = self.assign(self.inputs[1], a)
        ob = self.assign(self.output, b)
        for x, y in zip(ia, ob):
            self.copy(x.cell, y.cell)
        self.increment(len(ob))
        return ob

    def range_check(self, vals, rng):
        """layouts.rs:5024-5105: value into the first input VarTensor, its table-column index beside it in the second"""
        rc = self.base.range_checks[tuple(rng)]
        w = self.assign(self.inputs[0], vals)
        def col_index(v):
            s = v if v < R // 2 else v - R
            return abs(s - rc.range[0]) // rc.col_size
        self.assign(self.inputs[1], [Val(col_index(v.v)) for v in w])
        for t in range(len(w)):
            x, y, z = self.inputs[0].cartesian_coord(self.linear + t)
            self.enable(self.base.range_selectors[(tuple(rng), x, y)], z)
        self.increment(len(w))
        return w

    def _dup_inputs(self, var, vals):
        """assign_with_duplication_unconstrained: at a block boundary one row of filler (copies of the last value) is inserted"""
        bs, out, pos, used = var.block_size(), [], self.linear, 0
        for v in vals:
            out.append(self.put(var, pos, v))
            pos += 1; used += 1
            if pos % bs == 0:
                for _ in range(self.w):
                    self.put(var, pos, Val(v.v))
                    pos += 1; used += 1
        return out, used

    def dot(self, a, b):
        """layouts.rs:532-610: accumulated dot product, one row (w products) per step, DOTINIT then DOT with rotation -1"""
        assert len(a) == len(b)
        self.flush()
        w = self.w
        pad = (-len(a)) % w
        a, b = list(a) + [Val(0, const=True)] * pad, list(b) + [Val(0, const=True)] * pad
        ia, used = self._dup_inputs(self.inputs[0], a)
        ib, _ = self._dup_inputs(self.inputs[1], b)
        acc, pos, first, last = 0, self.linear, True, None
        for s in range(0, len(ia), w):
            acc = (acc + sum(x.v * y.v for x, y in zip(ia[s:s + w], ib[s:s + w]))) % R
            x, _, z = self.output.cartesian_coord(pos)
            if z == 0 and not first:                   # duplicate of the running sum at the top of a new column: no selector
                dup = self.put(self.output, pos, Val(last.v))
                self.copy(dup.cell, last.cell)
                pos += w
                x, _, z = self.output.cartesian_coord(pos)
            last = self.put(self.output, pos, Val(acc))
            self.enable(self.base.selectors[(EC.DOTINIT if first else EC.DOT, x, 0)], z)
            first = False
            pos += w
        self.increment(used)
        return last

    def _accumulate(self, vals, init_op, op, unit, fold):
        """layouts.rs:2472-2621 `sum` / `prod`: the tensor goes into the SECOND input VarTensor (padded to a whole row with the
        operation's unit), the running value into the output VarTensor one row per step, SUMINIT / CUMPRODINIT on the first row and
        SUM / CUMPROD (rotation -1) on the others, with the same duplicated rows at column boundaries as `dot`"""
        self.flush()
        w = self.w
        vals = list(vals) + [Val(unit, const=True)] * ((-len(vals)) % w)
        ib, used = self._dup_inputs(self.inputs[1], vals)
        acc, pos, first, last = unit, self.linear, True, None
        for s in range(0, len(ib), w):
            acc = fold(acc, [x.v for x in ib[s:s + w]])
            x, _, z = self.output.cartesian_coord(pos)
            if z == 0 and not first:                   # duplicate of the running value at the top of a new column: no selector
                dup = self.put(self.output, pos, Val(last.v))
                self.copy(dup.cell, last.cell)
                pos += w
                x, _, z = self.output.cartesian_coord(pos)
            last = self.put(self.output, pos, Val(acc))
            self.enable(self.base.selectors[(init_op if first else op, x, 0)], z)
            first = False
            pos += w
        self.increment(used)
        return last

    def sum(self, vals):
        if len(vals) == 1:
            return vals[0]
        return self._accumulate(vals, EC.SUMINIT, EC.SUM, 0, lambda acc, chunk: (acc + sum(chunk)) % R)

    def prod(self, vals):
        def fold(acc, chunk):
            for v in chunk:
                acc = acc * v % R
            return acc
        return self._accumulate(vals, EC.CUMPRODINIT, EC.CUMPROD, 1, fold)

    def decompose(self, vals, base, legs, zero_sign_matters=False):
        """layouts.rs:6321-6423: hints [sign, digits..] on the output VarTensor, range checks, recomposition by dot products with the base
        powers, multiplication by the sign, equality with the input.  zero_sign_matters (:6389-6403): is_zero(input) * sign == 0, between
        the two range checks -- a zero input must carry the sign 0"""
        if any(v.cell is None and not v.const for v in vals):
            vals = self.assign(self.inputs[0], vals)   # not yet assigned (model input / instance): placed without advancing
        hints = []
        for v in vals:
            s = v.v if v.v < R // 2 else v.v - R
            sg, mag = (s > 0) - (s < 0), abs(s)
            digs = [(mag // base ** (legs - 1 - t)) % base for t in range(legs)]
            assert mag < base ** legs, "value exceeds the decomposition range"
            hints += [Val(sg)] + [Val(d) for d in digs]
        claimed = self.assign(self.output, hints)
        self.increment(len(claimed))
        signs = [claimed[t] for t in range(0, len(claimed), legs + 1)]
        rest = [claimed[t] for t in range(len(claimed)) if t % (legs + 1)]
        signs = self.range_check(signs, (-1, 1))
        if zero_sign_matters:
            is_zero = self.equals_zero(vals)
            sign_is_zero = self.pairwise(signs, is_zero, EC.MULT)
            self.enforce_equality(sign_is_zero, [Val(0, const=True)] * len(sign_is_zero))
        rest = self.range_check(rest, (0, base - 1))
        bases = [Val(base ** (legs - 1 - t), const=True) for t in range(legs)]
        recomposed = [self.dot(rest[i * legs:(i + 1) * legs], bases) for i in range(len(vals))]
        signed = self.pairwise(recomposed, signs, EC.MULT)
        self.enforce_equality(vals, signed)
        return claimed, vals

    def equals_zero(self, vals):
        """layouts.rs:3549-3580"""
        inv = [Val(pow(v.v, -1, R) if v.v else 0) for v in vals]
        prod = self.pairwise(vals, inv, EC.MULT)
        out = self.pairwise([Val(1, const=True)] * len(vals), prod, EC.SUB)
        check = self.pairwise(vals, out, EC.MULT)
        self.enforce_equality(check, [Val(0, const=True)] * len(check))
        return out

    def relu(self, vals, base, legs):
        """leaky_relu with alpha = 0 (layouts.rs:6457-6474): sign by decomposition, mask = (sign == 1), x * mask"""
        claimed, vals = self.decompose(vals, base, legs)
        sign = [claimed[t] for t in range(0, len(claimed), legs + 1)]
        diff = self.pairwise(sign, [Val(1, const=True)] * len(sign), EC.SUB)
        mask = self.equals_zero(diff)
        return self.pairwise(vals, mask, EC.MULT)

    def sign(self, vals, zero_sign_matters=False):
        """layouts.rs:6425-6445: the sign hints of a decomposition at the region's base and legs"""
        base, legs = self.decomp
        claimed, _ = self.decompose(vals, base, legs, zero_sign_matters)
        return [claimed[t] for t in range(0, len(claimed), legs + 1)]

    def abs(self, vals):
        """layouts.rs:6447-6455"""
        return self.pairwise(vals, self.sign(vals), EC.MULT)

    def equals(self, a, b):
        """layouts.rs:3494-3501"""
        return self.equals_zero(self.pairwise(a, b, EC.SUB))

    def greater(self, a, b):
        """layouts.rs:3112-3128: sign(a - b) with the zero's sign pinned, then sign == 1"""
        sg = self.sign(self.pairwise(a, b, EC.SUB), True)
        return self.equals(sg, [Val(1, const=True)] * len(sg))

    def less(self, a, b):
        """layouts.rs:3236-3243"""
        return self.greater(b, a)

    def greater_equal(self, a, b):
        """layouts.rs:3161-3172: a + 1 > b"""
        return self.greater(self.pairwise(a, [Val(1, const=True)] * len(a), EC.ADD), b)

    def less_equal(self, a, b):
        """layouts.rs:3277-3284"""
        return self.greater_equal(b, a)

    def boolean_identity(self, vals):
        """layouts.rs:4885-4904 with assign = true: the values on the output VarTensor, and a (0, 1) range check of them"""
        out = self.assign(self.output, vals)
        self.increment(len(out))
        self.range_check(vals, (0, 1))
        return out

    def iff(self, mask, a, b):
        """layouts.rs:3818-3841: mask * a + (1 - mask) * b with the mask held to a boolean"""
        mask = self.boolean_identity(mask)
        rest = self.pairwise([Val(1, const=True)] * len(mask), mask, EC.SUB)
        return self.pairwise(self.pairwise(a, mask, EC.MULT), self.pairwise(b, rest, EC.MULT), EC.ADD)

    def and_(self, a, b):
        """layouts.rs:3345-3357 `and` (a keyword here): the product of two booleans"""
        return self.pairwise(self.boolean_identity(a), self.boolean_identity(b), EC.MULT)

    def or_(self, a, b):
        """layouts.rs:3414-3431 `or`: iff(a, a, b)"""
        return self.iff(a, a, self.boolean_identity(b))

    def l1_distance(self, a, b):
        """layouts.rs:58-67"""
        return self.abs(self.pairwise(a, b, EC.SUB))

    def diff_less_than(self, a, b, constant):
        """layouts.rs:156-172: |a - b| < constant, enforced"""
        distance = self.l1_distance(a, b)
        is_less = self.less(distance, [Val(constant, const=True)] * len(distance))
        self.enforce_equality(is_less, [Val(1, const=True)] * len(is_less))

    def div(self, vals, d):
        """layouts.rs:219-267, the rebase of a RebaseScale node with an integer denominator (HybridOp::Div, hybrid.rs:279-286): the prover
        claims the rounded quotient (`round_div`), the claim is range-checked by decomposition, and |input - claim * d| < d is enforced"""
        if d == 1:                                     # :225-227
            return vals
        claimed = [Val(round_div(signed(v.v), d)) for v in vals]
        base, legs = self.decomp
        _, claimed = self.decompose(claimed, base, legs)
        product = self.pairwise(claimed, [Val(d, const=True)] * len(claimed), EC.MULT)
        self.diff_less_than(vals, product, d)
        return claimed

    def nonlinearity(self, vals, name):
        """layouts.rs:5143-5222: x into the lookup input VarTensor, f(x) into the output VarTensor, the table-column index of x into
        the index VarTensor, the (op, block, inner column) selector on every row"""
        table = self.base.static_tables[name]
        w = self.assign(self.inputs[0], vals)
        signed = lambda v: v if v < R // 2 else v - R
        for v in w:
            assert table.range[0] <= signed(v.v) <= table.range[1], "lookup input %d outside the table range" % signed(v.v)
        self.lookup_inputs_seen([signed(v.v) for v in w])
        out = self.assign(self.output, [Val(table.f(signed(v.v)) % R) for v in w])
        self.assign(self.inputs[1], [Val((signed(v.v) - table.range[0]) // table.col_size) for v in w])
        for t in range(len(w)):
            x, y, z = self.inputs[0].cartesian_coord(self.linear + t)
            self.enable(self.base.static_selectors[(name, x, y)], z)
        self.increment(len(w))
        return out

    def lookup_inputs_seen(self, signed_inputs):
        """the statistics of `nonlinearity` (a recording region, whose values are symbols, keeps none)"""
        self.min_lookup_inputs = min(self.min_lookup_inputs, *signed_inputs)
        self.max_lookup_inputs = max(self.max_lookup_inputs, *signed_inputs)

    def _lookup_any(self, table_sel, input_sels, table_rows, picks, constrained=False):
        """the two sides of a lookup_any argument of BaseConfig::_configure_any (chip.rs:619-833): `table_rows` (3-tuples) go to the three
        single-column table VarTensors at the dynamic coordinate with the table selector on; `picks` go to (input 0, input 1, output) at
        the linear coordinate -- one tuple per cell position -- with that position's input selector on.  constrained: a Val that has a
        cell is copied from it and a constant is a constant (what `region.assign` does: a sort proves nothing about cells the argument
        does not read); otherwise the value alone is placed.  -> the table side as placed, row by row"""
        tabs = self.gc.advices[3:6]
        dyn = getattr(self, "dyn", 0)
        if constrained:
            free = lambda x: x if isinstance(x, Val) else Val(int(x), const=True)
        else:
            free = lambda x: Val(x.v) if isinstance(x, Val) else Val(int(x))     # the value alone: neither side of the argument is copy-constrained
        placed = []
        for r, tri in enumerate(table_rows):
            assert all(dyn + r < tabs[t].col_size for t in range(3)), "dynamic table column overflow"
            placed.append([self.put(tabs[t], dyn + r, free(tri[t])) for t in range(3)])      # one column per VarTensor: linear = row
            self.enable(table_sel, dyn + r)
        self.dyn = dyn + len(table_rows)
        self.dyn_table = (table_rows, placed)          # the table just written, cell by cell: what `row_at` picks of it read
        vars3 = [self.inputs[0], self.inputs[1], self.output]
        self.dyn_picks = []                            # the input side as placed, pick by pick: what `select` returns of it
        for j, tri in enumerate(picks):
            x, y, z = self.inputs[0].cartesian_coord(self.linear + j)
            self.dyn_picks.append([self.put(vars3[t], self.linear + j, free(tri[t])) for t in range(3)])
            self.enable(input_sels[(0, (x, y))], z)
        self.increment(len(picks))
        return placed

    def row_at(self, table_rows, index):
        """row `index` (a Val) of `table_rows`, as a pick of a dynamic lookup over that table whose keys are its positions 0 .. n - 1: a
        row chosen by a VALUE (an embedding gather).  The structure of the reference's `select` (layouts.rs:1483-1581): the table keys
        are the positions, the lookup key is the index."""
        s = signed(index.v)
        assert 0 <= s < len(table_rows), GATHER_ERROR
        return table_rows[s]

    def dynamic_lookup(self, table_rows, picks):
        """layouts.rs `dynamic_lookup`: every pick is a row of the table (a gather / embedding lookup)"""
        self._lookup_any(self.base.dynamic_table_selectors[0], self.base.dynamic_lookup_selectors, table_rows, picks)

    def shuffle(self, rows, order):
        """layouts.rs `shuffles`: the inputs are the rows of the reference side in another order (sort / transpose)"""
        self._lookup_any(self.base.shuffle_output_selectors[0], self.base.shuffle_input_selectors, rows, [rows[i] for i in order])

    def _sorted(self, vals, mode):
        """the one data-dependent step of a sort: -> (the values in ascending order, the position each came from).  The order is by (signed
        value, position), the position ascending -- descending for `largest_index_first` -- among equal values: what the claimed-index
        search of `shuffles` (layouts.rs:1662-1704: the first unused position in input order, reversed for the third mode) yields, the
        only witness the indexed modes accept, and a total order.  (A recording region overrides this, as it overrides `row_at`.)"""
        s = [signed(v.v) for v in vals]
        for x in s:
            assert abs(x) < 1 << 62, SORT_ERROR
        order = sorted(range(len(s)), key=lambda j: (s[j], -j if mode == "largest_index_first" else j))
        return [s[j] % R for j in order], order

    def sort_ascending(self, vals, mode="unsorted"):
        """layouts.rs:1158-1275 `_sort_ascending` -> (sorted, indices): the sorted values on the first input VarTensor, the permutation
        argument of `shuffles` (:1624-1760) -- table side (sorted_i, the region's shuffle index, the claimed source index_i), input side
        (input_j, the same constant, j) -- and the ordering constraints of the collision mode over consecutive pairs"""
        assert mode in SORT_MODES, mode
        vals = list(vals)
        if len(vals) == 1:                             # :1167-1169
            return vals, [Val(0, const=True)]
        values, positions = self._sorted(vals, mode)
        srt = self.assign(self.inputs[0], [Val(v) for v in values])
        self.increment(len(srt))
        index = Val(self.shuffle_index, const=True)
        placed = self._lookup_any(self.base.shuffle_output_selectors[0], self.base.shuffle_input_selectors,
                                  [(srt[i], index, Val(positions[i])) for i in range(len(srt))],
                                  [(v, index, Val(j, const=True)) for j, v in enumerate(vals)], constrained=True)
        self.shuffle_index += 1
        idx = [row[2] for row in placed]               # the claimed indices, where the argument reads them
        a, b, ia, ib = srt[:-1], srt[1:], idx[:-1], idx[1:]
        if mode == "unsorted":
            ordered = self.greater_equal(b, a)
        else:                                          # strictly ascending, or equal with the source indices in the mode's order
            greater, equal = self.greater(b, a), self.equals(b, a)
            by_index = self.greater(ib, ia) if mode == "smallest_index_first" else self.less(ib, ia)
            ordered = self.or_(greater, self.and_(equal, by_index))
        self.enforce_equality([Val(1, const=True)] * len(ordered), ordered)
        return srt, idx

    def topk(self, vals, k, largest=True):
        """layouts.rs:1298-1315 `_select_topk`: an `unsorted` sort, reversed for the largest, its first k"""
        srt, _ = self.sort_ascending(vals, "unsorted")
        return (srt[::-1] if largest else srt)[:k]

    def topk_axes(self, rows, k, largest=True):
        """layouts.rs:1343-1361 `topk_axes` over a list of equal-length rows (the slices along the axis)"""
        return [self.topk(row, k, largest) for row in rows]

    def not_(self, mask):
        """layouts.rs:3727-3740 `not` (a keyword here): iff(mask, 0, 1)"""
        n = len(mask)
        return self.iff(mask, [Val(0, const=True)] * n, [Val(1, const=True)] * n)

    def optimum_convex_function(self, x, f):
        """layouts.rs:114-143: 1 where x is the smallest minimiser of the convex f over the integers: f(x) <= f(x + 1) and f(x) < f(x - 1)"""
        one = [Val(1, const=True)] * len(x)
        f_x = f(x)
        f_x_plus_1 = f(self.pairwise(x, one, EC.ADD))
        f_x_minus_1 = f(self.pairwise(x, one, EC.SUB))
        is_opt_rhs = self.less_equal(f_x, f_x_plus_1)
        is_opt_lhs = self.less(f_x, f_x_minus_1)
        return self.and_(is_opt_lhs, is_opt_rhs)

    def recip(self, vals, input_scale, output_scale, eps):
        """layouts.rs:300-385: the prover claims round(input_scale * output_scale / x) (`recip_claim`), the claim is range-checked by
        decomposition, a zero input is held to `zero_inverse` = round(output_scale / eps) by the two masks, and everywhere else the claim
        must minimise |claim * x - input_scale * output_scale|"""
        n = len(vals)
        S = int(input_scale) * int(output_scale)
        zero_inverse = zero_recip(output_scale, eps)
        claimed = [Val(recip_claim(signed(v.v), S, zero_inverse)) for v in vals]
        base, legs = self.decomp
        _, claimed = self.decompose(claimed, base, legs)
        equal_zero_mask = self.equals_zero(vals)
        not_equal_zero_mask = self.not_(equal_zero_mask)
        equal_inverse_mask = self.equals(claimed, [Val(zero_inverse, const=True)] * n)
        masked_unit_scale = self.pairwise([Val(S, const=True)] * n, not_equal_zero_mask, EC.MULT)
        self.enforce_equality(equal_zero_mask, equal_inverse_mask)
        def err_func(x):
            return self.l1_distance(self.pairwise(x, vals, EC.MULT), masked_unit_scale)
        is_opt = self.optimum_convex_function(claimed, err_func)
        is_opt = self.pairwise(is_opt, equal_zero_mask, EC.ADD)           # a zero input is excused from the optimum
        self.enforce_equality(is_opt, [Val(1, const=True)] * n)
        return claimed

    def sqrt(self, vals, input_scale):
        """layouts.rs:408-459: the prover claims round(sqrt(x * input_scale)) (`sqrt_claim`), `abs` holds the claim to its range and to a
        sign, and the claim must minimise |claim^2 - x * input_scale|"""
        n = len(vals)
        claimed = [Val(sqrt_claim(signed(v.v), int(input_scale))) for v in vals]
        claimed = self.abs(claimed)
        rescaled_input = self.pairwise(vals, [Val(int(input_scale), const=True)] * n, EC.MULT)
        def err_func(x):
            return self.l1_distance(self.pairwise(x, x, EC.MULT), rescaled_input)
        is_opt = self.optimum_convex_function(claimed, err_func)
        self.enforce_equality(is_opt, [Val(1, const=True)] * n)
        return claimed

    def rsqrt(self, vals, input_scale, output_scale, eps):
        """layouts.rs:482-505: the reciprocal of the square root"""
        return self.recip(self.sqrt(vals, input_scale), input_scale, output_scale, eps)

    def max(self, vals):
        """layouts.rs:5390-5400: the last of an `unsorted` ascending sort"""
        return self.sort_ascending(vals, "unsorted")[0][-1]

    def min(self, vals):
        """layouts.rs:5403-5413: the first of an `unsorted` ascending sort"""
        return self.sort_ascending(vals, "unsorted")[0][0]

    def percent(self, vals, input_scale, output_scale, eps):
        """layouts.rs:6632-6661: every value times the reciprocal of their sum"""
        if any(v.cell is None and not v.const for v in vals):
            vals = self.assign(self.inputs[0], vals)
            self.increment(len(vals))
        denom = self.sum(vals)
        inv_denom = self.recip([denom], input_scale, output_scale, eps)
        return self.pairwise(vals, [inv_denom[0]] * len(vals), EC.MULT)

    def softmax(self, vals, input_scale, output_scale, eps, exp="exp"):
        """layouts.rs:6687-6711: the maximum is subtracted, the static lookup `exp` (LookupOp::Exp at the input scale) is applied, `percent`"""
        max_val = self.max(vals)
        sub = self.pairwise(vals, [max_val] * len(vals), EC.SUB)
        ex = self.nonlinearity(sub, exp)
        return self.percent(ex, input_scale, output_scale, eps)

    def softmax_axes(self, rows, input_scale, output_scale, eps, exp="exp"):
        """layouts.rs:6610-6629 `softmax_axes` over a list of equal-length rows (the slices along the axis)"""
        return [self.softmax(row, input_scale, output_scale, eps, exp) for row in rows]

    def mean_of_squares(self, rows):
        """layouts.rs:3022-3035 `mean_of_squares_axes` over a list of equal-length rows: the squares (`pow` 2: `pairwise` MULT with itself),
        their sum per row, `div` by the row length -> one value per row"""
        length = len(rows[0])
        flat = [v for row in rows for v in row]
        squared = self.pairwise(flat, flat, EC.MULT)
        sum_squared = [self.sum(squared[i * length:(i + 1) * length]) for i in range(len(rows))]
        return self.div(sum_squared, length)

    def _arg_extremum(self, vals, mode):
        """the one data-dependent step of `argmax` / `argmin`: the SMALLEST position whose signed value is the greatest (mode "max") or the
        least ("min") -- the reference's `max_by_key((value, -idx))` / `min_by_key((value, idx))` (layouts.rs:5231-5237, :5265-5271), and the
        only claim the gates accept: the sort that checks it is `largest_index_first` with the claim held to its LAST index for the maximum,
        `smallest_index_first` with the claim held to its FIRST for the minimum.  (A recording region overrides this, as it overrides
        `_sorted`.)"""
        assert mode in ("max", "min"), mode
        s = [signed(v.v) for v in vals]
        for x in s:
            assert abs(x) < 1 << 62, ARGEXT_ERROR
        return s.index(max(s) if mode == "max" else min(s))

    def select(self, vals, index):
        """layouts.rs:1363-1396 `select`: the element of `vals` the cell `index` names, through a dynamic lookup (:1483-1581) -- table side
        (the position as a constant, vals_j, the region's dynamic-lookup index), input side (the index cell, the claimed element, the same
        constant).  -> the claimed element where the argument reads it"""
        lookup_index = Val(self.dynamic_lookup_index, const=True)
        table_rows = [(Val(j, const=True), v, lookup_index) for j, v in enumerate(vals)]
        row = self.row_at(table_rows, index)
        pick = (Val(row[0].v, index.cell), Val(row[1].v), lookup_index)
        self._lookup_any(self.base.dynamic_table_selectors[0], self.base.dynamic_lookup_selectors, table_rows, [pick], constrained=True)
        self.dynamic_lookup_index += 1
        return self.dyn_picks[0][1]

    def _arg(self, vals, mode):
        vals = list(vals)
        claim = self.assign(self.inputs[1], [Val(self._arg_extremum(vals, mode))])      # "this is safe because we later constrain it"
        self.increment(1)
        claimed_val = self.select(vals, claim[0])
        srt, idx = self.sort_ascending(vals, "largest_index_first" if mode == "max" else "smallest_index_first")
        at = -1 if mode == "max" else 0
        self.enforce_equality([claimed_val], [srt[at]])
        self.enforce_equality(claim, [idx[at]])
        return claim[0]

    def argmax(self, vals):
        """layouts.rs:5225-5256: the claimed index on the second input VarTensor, `select` of it, a `largest_index_first` sort, and the
        claimed element and index held to the sort's last value and last index"""
        return self._arg(vals, "max")

    def argmin(self, vals):
        """layouts.rs:5259-5293: as `argmax` with a `smallest_index_first` sort and its first value and first index"""
        return self._arg(vals, "min")

    def argmax_axes(self, rows):
        """layouts.rs:2781-2856 `argmax_axes` over a list of equal-length rows (the slices along the axis)"""
        return [self.argmax(row) for row in rows]

    def argmin_axes(self, rows):
        """layouts.rs:2859-2905 `argmin_axes` over a list of equal-length rows"""
        return [self.argmin(row) for row in rows]

    @staticmethod
    def _padded(image, channels, height, width, padding):
        """`Tensor::pad` over the two spatial axes of a canonical (batch 1) NCHW image given row-major: zeros as constants, padding =
        ((top, bottom), (left, right)) -> (the padded image as [channel][row][column], its height, its width)"""
        assert len(image) == channels * height * width
        (top, bottom), (left, right) = padding
        zero = Val(0, const=True)
        H, W = top + height + bottom, left + width + right
        out = [[[image[(c * height + i - top) * width + j - left] if top <= i < top + height and left <= j < left + width else zero
                 for j in range(W)] for i in range(H)] for c in range(channels)]
        return out, H, W

    def max_pool(self, image, channels, height, width, padding, stride, pool):
        """layouts.rs:4008-4087 on a canonical NCHW image of batch 1: zero padding, then one `max` per output position in the order of the
        cartesian product (channel, row, column) -> the pooled image, row-major"""
        img, H, W = self._padded(image, channels, height, width, padding)
        slides = [(H - pool[0]) // stride[0] + 1, (W - pool[1]) // stride[1] + 1]
        return [self.max([img[c][i * stride[0] + a][j * stride[1] + b] for a in range(pool[0]) for b in range(pool[1])])
                for c in range(channels) for i in range(slides[0]) for j in range(slides[1])]

    def sumpool(self, image, channels, height, width, padding, stride, kernel, normalized):
        """layouts.rs:3907-3980 on a canonical NCHW image of batch 1: the unit kernel is assigned once on the second input VarTensor, every
        channel is convolved with it (`conv`, :4499-4661, without a bias: one `dot` of each window with the kernel cells) and the sums are
        divided by the kernel size when `normalized` -> the pooled image, row-major"""
        img, H, W = self._padded(image, channels, height, width, padding)
        unit = self.assign(self.inputs[1], [Val(1, const=True)] * (kernel[0] * kernel[1]))
        self.increment(len(unit))
        slides = [(H - kernel[0]) // stride[0] + 1, (W - kernel[1]) // stride[1] + 1]
        out = []
        for c in range(channels):
            for i in range(slides[0]):
                for j in range(slides[1]):
                    out.append(self.dot([img[c][i * stride[0] + a][j * stride[1] + b] for a in range(kernel[0]) for b in range(kernel[1])], unit))
                    self.flush()
        return self.div(out, kernel[0] * kernel[1]) if normalized else out

    def conv(self, kernels, image, bias, channels, side, kernel, stride):
        """layouts.rs:4499-4661 of ONE input channel, a square `side` x `side` image and `channels` square filters, all row-major: kernels
        and image are assigned once, side by side (every patch / filter slice below is a copy of those cells); then per output, in the
        order (channel, row, column), one `dot` of the patch with the filter and the channel's bias added.  bias(o) -> the Val of channel
        o's bias, asked for at every output position -> the outputs, row-major"""
        K, slides = kernel, (side - kernel) // stride + 1
        ker = self.assign(self.inputs[0], kernels)
        im = self.assign(self.inputs[1], image)
        self.increment(max(len(ker), len(im)))
        out = []
        for o in range(channels):
            for i in range(slides):
                for j in range(slides):
                    patch = [im[(i * stride + a) * side + j * stride + b] for a in range(K) for b in range(K)]
                    res = self.pairwise([self.dot(patch, ker[o * K * K:(o + 1) * K * K])], [bias(o)], EC.ADD)
                    self.flush()
                    out.append(res[0])
        return out

    # ---- the indexed family: gather, scatter, one-hot ---------------------------------------------------------------------------------
    def select_elements(self, vals, indices):
        """layouts.rs:1363-1396 `select` for many picks in ONE dynamic lookup (:1483-1581): table side (the position as a constant, vals_j,
        the region's dynamic-lookup index), input side one pick per index cell (the index cell, the claimed element, the same constant),
        constrained as `select` does it.  -> the claimed elements where the argument reads them"""
        lookup_index = Val(self.dynamic_lookup_index, const=True)
        table_rows = [(Val(j, const=True), v, lookup_index) for j, v in enumerate(vals)]
        picks = []
        for index in indices:
            row = self.row_at(table_rows, index)
            picks.append((Val(row[0].v, index.cell, index.const), Val(row[1].v), lookup_index))
        self._lookup_any(self.base.dynamic_table_selectors[0], self.base.dynamic_lookup_selectors, table_rows, picks, constrained=True)
        self.dynamic_lookup_index += 1
        return [pick[1] for pick in self.dyn_picks]

    @staticmethod
    def _strides(dims):
        """the row-major multiplier of every dimension (`dim_multiplier`, layouts.rs:1947-1956)"""
        out, acc = [], 1
        for d in reversed(dims):
            out.append(acc)
            acc *= d
        return out[::-1]

    @staticmethod
    def _coords(dims):
        """the coordinates of `dims` in row-major order (`multi_cartesian_product`)"""
        return [tuple(int(c) for c in coord) for coord in np.ndindex(*dims)]

    def linearize_element_index(self, index, dims, dim, is_flat_index, index_dims=None):
        """layouts.rs:1924-2012: the position in the flattened tensor of shape `dims` each index names along `dim` -- per element a
        `pairwise` MULT by the constant multiplier of `dim` and a `pairwise` ADD of the constant offset of the other coordinates.  A flat
        index (`gather`) is iterated over dims with dims[dim] = len(index); otherwise `index` has the shape `index_dims`, of the rank of
        `dims`, and an index of rank 1 is returned as it is (:1942-1944)"""
        dims = list(dims)
        if not is_flat_index:
            index_dims = [len(index)] if index_dims is None else list(index_dims)
            assert len(index_dims) == len(dims)
            if len(index_dims) == 1:
                return list(index)
        mult = self._strides(dims)
        iteration_dims = dims[:dim] + [len(index)] + dims[dim + 1:] if is_flat_index else index_dims
        out = []
        for i, coord in enumerate(self._coords(iteration_dims)):
            index_val = index[coord[dim]] if is_flat_index else index[i]
            const_offset = sum(coord[t] * mult[t] for t in range(len(dims)) if t != dim)
            res = self.pairwise([index_val], [Val(mult[dim], const=True)], EC.MULT)
            out.append(self.pairwise(res, [Val(const_offset, const=True)], EC.ADD)[0])
        return out

    def gather(self, vals, dims, index, dim):
        """layouts.rs:1822-1847: the slices of the tensor `vals` (shape `dims`, row-major) the flat `index` names along `dim` -> the output,
        row-major, of shape dims with dims[dim] = len(index)"""
        return self.select_elements(vals, self.linearize_element_index(index, dims, dim, True))

    def gather_elements(self, vals, dims, index, index_dims, dim):
        """layouts.rs:1850-1870: out[coord] = vals[coord with coord[dim] = index[coord]] over the shape of the index -> (output, linear index)"""
        assert len(dims) == len(index_dims)
        linear = self.linearize_element_index(index, dims, dim, False, index_dims)
        return self.select_elements(vals, linear), linear

    def _one_hot(self, s, num_classes):
        """the one data-dependent step of `one_hot`: the vector with a one at the signed index s (`tensor::ops::one_hot`).  (A recording
        region overrides this, as it overrides `_sorted`.)"""
        assert 0 <= s < num_classes and abs(s) < 1 << 62, ONEHOT_ERROR
        return [int(j == s) for j in range(num_classes)]

    def one_hot(self, index, num_classes):
        """layouts.rs:1398-1442 for one index cell: the claimed vector, `boolean_identity` of it with the index assigned beside it on the
        first input VarTensor and the `max(len)` increment, `sum` == 1, and `gather` of the claim at the index == 1"""
        claim = [Val(v) for v in self._one_hot(signed(index.v), num_classes)]
        assigned_input = self.assign(self.inputs[0], [index])
        assigned_output = self.boolean_identity(claim)
        self.increment(max(len(assigned_output), len(assigned_input)))
        unit = [Val(1, const=True)]
        self.enforce_equality(unit, [self.sum(assigned_output)])
        gathered = self.gather(assigned_output, [num_classes], assigned_input, 0)
        self.enforce_equality(unit, gathered)
        return assigned_output

    def one_hot_axis(self, index, dims, num_classes, dim):
        """layouts.rs:1769-1819 over the flat list of the index cells of a tensor of shape `dims`: one `one_hot` per cell, in order, arranged
        into the shape dims with `num_classes` inserted at `dim` -> the output, row-major"""
        dims = list(dims)
        assert len(index) == int(np.prod(dims, dtype=np.int64))
        ops = [self.one_hot(cell, num_classes) for cell in index]
        strides = self._strides(dims)
        out = []
        for coord in self._coords(dims[:dim] + [num_classes] + dims[dim:]):
            op_idx = coord[:dim] + coord[dim + 1:]
            out.append(ops[sum(c * s for c, s in zip(op_idx, strides))][coord[dim]])
        return out

    def _claimed_indices(self, output, input):
        """the one data-dependent step of `shuffles` over an arbitrary input side (layouts.rs:1662-1704, `unsorted`): for every output
        element in turn the first position of the input, in input order, that holds its value and is not yet used; 0 where there is none
        (`unwrap_or(&0)`: the permutation then cannot hold).  (A recording region overrides this, as it overrides `_sorted`.)"""
        places = {}
        for j, v in enumerate(input):
            places.setdefault(signed(v.v), []).append(j)
        taken = {}
        out = []
        for v in output:
            x = signed(v.v)
            at, mine = taken.get(x, 0), places.get(x, ())
            out.append(mine[at] if at < len(mine) else 0)
            taken[x] = at + 1
        return out

    def shuffles(self, output, input):
        """layouts.rs:1624-1760 in `unsorted` mode: `output` is a permutation of `input` -- table side (output_i, the region's shuffle index,
        the claimed source index_i), input side (input_j, the same constant, j) -> the claimed indices where the argument reads them"""
        assert len(output) == len(input)
        index = Val(self.shuffle_index, const=True)
        claimed = self._claimed_indices(output, input)
        placed = self._lookup_any(self.base.shuffle_output_selectors[0], self.base.shuffle_input_selectors,
                                  [(o, index, Val(c)) for o, c in zip(output, claimed)],
                                  [(v, index, Val(j, const=True)) for j, v in enumerate(input)], constrained=True)
        self.shuffle_index += 1
        return [row[2] for row in placed]

    def _missing(self, vals, fullset):
        """the one data-dependent step of `get_missing_set_elements` (layouts.rs:2229-2244): the first occurrence in `fullset` of each input
        value in turn is deleted, the first len(fullset) - len(vals) of what remains are kept.  It never fails: a value not in the set
        deletes nothing.  (A recording region overrides this, as it overrides `_sorted`.)"""
        full = [signed(v.v) for v in fullset]
        places = {}
        for j, x in enumerate(full):
            places.setdefault(x, []).append(j)
        taken, gone = {}, [False] * len(full)
        for v in vals:
            x = signed(v.v)
            at, mine = taken.get(x, 0), places.get(x, ())
            if at < len(mine):
                gone[mine[at]] = True
                taken[x] = at + 1
        rest = [x for x, g in zip(full, gone) if not g]
        return [x % R for x in rest[:max(len(full) - len(vals), 0)]]

    def get_missing_set_elements(self, vals, fullset, ordered):
        """layouts.rs:2213-2286: the elements of `fullset` (distinct values) that `vals` lacks -- the claim on the output VarTensor, the
        permutation argument of `shuffles` with output side vals ++ claim and input side fullset, then an `unsorted` ascending sort of the
        claim when `ordered` (an empty claim has nothing to sort)"""
        vals = list(vals)
        claim = self.assign(self.output, [Val(v) for v in self._missing(vals, fullset)])
        self.increment(len(claim))
        self.shuffles(vals + claim, fullset)
        if ordered and claim:
            claim = self.sort_ascending(claim, "unsorted")[0]
        return claim

    def _scattered(self, input, index, src, dims, index_dims, dim):
        """the one data-dependent step of `scatter_elements`, `tensor::ops::scatter` (/root/reference/src/tensor/ops.rs:744-778): a copy of the
        input, then the elements of `src` (shape `index_dims`) in row-major order, each to its own coordinate with the one along `dim`
        replaced by its index: a later element overwrites an earlier one at the same target.  An index outside [0, dims[dim]) -- or beyond
        62 bits -- is the failure SCATTER_ERROR.  (A recording region overrides this, as it overrides `_sorted`.)"""
        assert len(index) == len(src) and all(a <= b for t, (a, b) in enumerate(zip(index_dims, dims)) if t != dim)
        out = [v.v for v in input]
        mult = self._strides(dims)
        for coord, i, v in zip(self._coords(index_dims), index, src):
            s = signed(i.v)
            assert 0 <= s < dims[dim] and abs(s) < 1 << 62, SCATTER_ERROR
            out[s * mult[dim] + sum(coord[t] * mult[t] for t in range(len(dims)) if t != dim)] = v.v
        return out

    def scatter_elements(self, input, dims, index, index_dims, src, dim):
        """layouts.rs:2313-2379, step for step: the index is assigned if it is not yet cells; the scattered tensor is CLAIMED on the output
        VarTensor (`_scattered`); `gather_elements` of the claim at the index is held equal to `src`; the positions the index does not
        name -- `get_missing_set_elements` of the linear index in the constants 0 .. n - 1, ordered -- are gathered from the flat claim
        and looked up, with their positions, in (position, input): what was not written is the input's.  -> the claim.
        Two elements on one target make the permutation argument unsatisfiable (the claim itself takes the later source)."""
        assert len(dims) == len(index_dims) and len(input) == int(np.prod(dims, dtype=np.int64))
        index = list(index)
        if not all(v.cell is not None for v in index):                   # :2323-2326
            index = self.assign(self.inputs[1], index)
            self.increment(len(index))
        claimed = self.assign(self.output, [Val(v) for v in self._scattered(input, index, src, dims, index_dims, dim)])
        self.increment(len(claimed))
        gather_src, linear_index = self.gather_elements(claimed, dims, index, index_dims, dim)
        self.enforce_equality(gather_src, list(src))
        full_index_set = [Val(j, const=True) for j in range(len(input))]
        input_indices = self.get_missing_set_elements(linear_index, full_index_set, True)
        gather_input, _ = self.gather_elements(claimed, [len(claimed)], input_indices, [len(input_indices)], 0)
        lookup_index = Val(self.dynamic_lookup_index, const=True)
        self._lookup_any(self.base.dynamic_table_selectors[0], self.base.dynamic_lookup_selectors,
                         [(j, v, lookup_index) for j, v in zip(full_index_set, input)],
                         [(i, g, lookup_index) for i, g in zip(input_indices, gather_input)], constrained=True)
        self.dynamic_lookup_index += 1
        return claimed

    def einsum(self, ein, A, B, challenges=None):
        """assign_einsum of an EinsumMatmulCircuit laid over this region's configuration (EinsumMatmulCircuit.over), in this region, at
        the einsum coordinate: A, B are len x len Vals.  Of an EinsumCircuit (EinsumCircuit.over): A, B are the operands as flat
        row-major lists of Vals, which may hold a cell already (`_assign` copy-constrains it), and the product comes back as Vals that
        carry the cell the claim landed in -- the first-phase RLC input column, at the rows of `assign_output`'s first RLC -- so that
        a later op that places the product is tied to it.  (The reference returns bare values here, layouts.rs:879: a deliberate
        superset of its copy constraints.)"""
        if isinstance(ein, EinsumCircuit):
            a, b = ([signed(v.v) for v in M] for M in (A, B))
            return ein.sequence(self, [list(A), list(B)], *ein.host_ops(a, b, challenges))
        ints = lambda M: np.array([[signed(v.v) for v in row] for row in M], np.int64)
        ein.sequence(self, A, B, *ein.host_ops(ints(A), ints(B), challenges))

    def constrain_instance(self, vals, inst_col, inst_offset=0):
        """Layouter::constrain_instance: the cells are tied to the instance column directly (what a hand-written halo2 circuit does)"""
        for t, v in enumerate(vals):
            self.copy(v.cell, ("inst", inst_col.index, inst_offset + t))

    def output_equals_instance(self, vals, inst_col, inst_offset, base, legs, decomp=True):
        """layouts.rs:6740-6779 `output`: range check (decompose) the outputs and the instance cells, then equality"""
        if decomp:
            _, vals = self.decompose(vals, base, legs)
        inst = []
        for t, v in enumerate(vals):                   # assign_advice_from_instance: the advice copy is tied to the instance cell
            inst.append(Val(v.v, ("inst", inst_col.index, inst_offset + t)))
        if decomp:
            inst = self.assign(self.inputs[0], inst)    # `!all_prev_assigned()`: an advice copy of the instance cells, placed without advancing
            _, inst = self.decompose(inst, base, legs)
        return self.enforce_equality(vals, inst)


class LayoutCircuit:
    """what every circuit built on BaseRegion shares: the synthesis pass over its `layout(reg, inputs, param[, challenges]) -> outputs`,
    the keygen pass (selector activations, fixed columns, copy constraints) and the witness pass.  Subclasses give `layout`, `n_inputs`,
    `plan_identity()` and `config()`: the constructor's keyword arguments, read off the attributes as they are now -- the ONE statement
    of a family's fields, which `fresh()` and execute.describe go through.
    What witness_plan asks of a circuit's class: plan_domain, the prefix of its params_hash (None: b"layout:<ClassName>:"; the empty one
    marks the MLP family, whose hashes and blobs stay what they were before plans held lookups); plan_tables, whether the static lookup
    tables are hashed in; lays_einsums, whether it lays Freivalds einsums over its own configuration (second-phase advice, a plan with
    phases)."""
    plan_domain, plan_tables, lays_einsums = None, True, False

    def synthesize(self, x, witness=True, challenges=None):
        """one pass of `layout` over a BaseRegion with the values of x (any shape, row-major) -> the region; sets self.outputs.
        challenges: given to a layout with phases (None lays its first phase only)"""
        x = np.asarray(x, dtype=object).reshape(-1).tolist()
        assert len(x) == self.n_inputs
        reg = BaseRegion(self.gc, witness)
        outs = self.layout(reg, [Val(int(v)) for v in x], lambda v: Val(int(v)), *(() if challenges is None else (challenges,)))
        reg.finish(self.gc.const_cols)
        self.outputs = [v.v for v in outs]
        return reg

    def fresh(self):
        """the same circuit, its fields and parameters as they are now, with an untouched constraint system (compress_selectors
        rewrites a system in place)"""
        return type(self)(**self.config())

    def keygen_inputs(self, x, with_witness=False):
        """-> (plonk.ConstraintSystem, fixed columns (lists of ints), copies over cs.perm positions, region); with_witness: ONE synthesis
        pass that also fills the advice columns (region.advice; `witness_of(region)` returns them) -- halo2 runs keygen and proving as
        separate passes, a benchmark that needs both can share one"""
        reg = self.synthesize(x, witness=with_witness)
        n = 1 << self.k
        cs0 = self.gc.cs
        rows = reg.selector_rows(dense=False)
        if all(a is None for a in rows):               # no selector is ever on (a sort of one element): the columns still have n rows
            rows = reg.selector_rows()
        sel_cols = cs0.compress_selectors(rows)
        if n <= 1 << 12:
            sel_cols = [c.tolist() for c in sel_cols]
        cs = cs0.to_plonk(self.k)
        tabs = self.gc.table_columns()
        n_pre = cs.n_fixed - len(sel_cols)
        fixed = [tabs.get(c) or reg.fixed.get(c) or [0] * n for c in range(n_pre)] + list(sel_cols)
        pos = {kc: i for i, kc in enumerate(cs.perm)}
        copies = [((pos[(a[0], a[1])], a[2]), (pos[(b[0], b[1])], b[2])) for a, b in reg.copies]
        return cs, fixed, copies, reg

    def witness(self, x):
        """advice columns (lists of ints) and the instance column"""
        return self.witness_of(self.synthesize(x, witness=True))

    def witness_of(self, reg):
        n = 1 << self.k
        adv = [reg.advice.get(c.index) or [0] * n for c in self.gc.cs.advice]
        return adv, [self.outputs]

    def instances(self, x, outputs=None):
        """the instance columns of a witness: the public output (None: that of the last synthesis)"""
        return [list(self.outputs if outputs is None else outputs)]


def _decomposition_cells(m, w, legs):
    """the cells `decompose` places for m values: hints, the two range checks, the recomposing dots, MULT by the sign, the equality"""
    return m * (legs + 1) + m + m * legs + m * (-(-legs // w) * w) + 2 * m


DEFAULT_VISIBILITY = ("Private", "Private", "Public")
VISIBILITIES = (("Private", "Public", "KZGCommit"), ("Private", "Fixed", "KZGCommit"), ("Public", "KZGCommit"))     # input, params, output


def visibility_triple(vis):
    """(input, params, output) of an MlpCircuit, checked: None is the default triple; a dict with those keys or a sequence of three.
    Refused by name, as a ValueError: anything Hashed (a dict, as ezkl's Visibility::Hashed deserialises), a Fixed input or output, a
    Private output, and whatever else is outside VISIBILITIES."""
    if vis is None:
        return DEFAULT_VISIBILITY
    if isinstance(vis, dict):
        vis = (vis.get("input", "Private"), vis.get("params", "Private"), vis.get("output", "Public"))
    vis = tuple(vis)
    if len(vis) != 3:
        raise ValueError("a visibility triple is (input, params, output)")
    for what, v, accepted in zip(("input", "params", "output"), vis, VISIBILITIES):
        if isinstance(v, dict) or v == "Hashed":
            raise ValueError("unsupported visibility: %s is Hashed (Poseidon modules are outside this package's scope)" % what)
        if v not in accepted:
            raise ValueError("unsupported visibility: %s is %s (the mlp family takes an input that is %s, parameters that are %s and an output that is %s)"
                             % ((what, v if isinstance(v, str) else repr(v)) + tuple(", ".join(a[:-1]) + " or " + a[-1] for a in VISIBILITIES)))
    return vis


class MlpCircuit(LayoutCircuit):
    """`layers` x (Gemm + bias + ReLU) on one input vector, the op sequence of the reference's fixture model
    (tests/assets/network.onnx: Gemm 3 -> 4 + ReLU) and of examples/onnx/large_mlp/gen.py:6-43 (9 x Linear(100, 100) + ReLU; with
    batch 1 the einsum "mk,nk->mn" has one non-common index and is laid out with base ops, einsum/analysis.rs:165-184), inputs /
    outputs range-checked by decomposition (src/graph/model.rs:1132-1258).  By default private input and parameters and a public
    output; `visibility` = (input, params, output) chooses among VISIBILITIES, as GraphCircuit::synthesize does (src/graph/mod.rs:2010-2200):

      KZGCommit   the tensor is assigned, from row 0 and without duplication, to unblinded advice columns of its own that come BEFORE the
                  model's (GraphConfig.polycommit, in the order input, params, output; all parameters are ONE tensor, in the order `layout`
                  asks for them: per layer the weight rows, then the bias -- `flat_params`); the model reads those cells in place of the raw
                  values (an input / a parameter: copy constraints from the module's cells; the outputs: copy constraints to the model's
                  cells, and no `output` op).  The commitment to such a column is what PolyCommitChip::commit computes outside the
                  circuit, and the first points of a proof.
                  (The reference hands a constant that ONE node uses to the model as a bare value, src/graph/model.rs:1323-1330, which
                  leaves it untied to the module; here every parameter is read from the module's cell.)
      Public      input: the single instance column holds the input first, the output after it; the model's first use of the input
                  assigns it from the instance (assign_advice_from_instance), the output comparison moves to offset n_inputs
      Fixed       params: every parameter is a ValType::Constant -- placed through the region's constant cache (one fixed cell per
                  distinct value, shared with the layout's own constants; BaseRegion.put / finish), so the parameters are part of the key

    `instances(x)` is the instance column of a witness (prepare_public_inputs, src/graph/mod.rs:1411-1446)."""
    plan_domain = b""

    def __init__(self, logrows, num_inner_cols, weights, biases, decomp_base, decomp_legs, total_assignments=None, relu_last=True,
                 n_inputs=None, relu_first=False, rebase=None, visibility=None, total_const_size=None):
        """rebase: one positive integer per layer, the denominator of the RebaseScale that wraps the layer's Einsum node (node.rs:143-205:
        `div` of the Gemm's output, before the bias is added; 1 = the layer is not rescaled), or None for none.
        relu_first / n_inputs: a LeakyReLU (slope 0) straight on the input, before any Gemm -- with no layers at all that is
        examples/onnx/1l_relu (gen.py: nn.ReLU on a vector of 3), BASELINE configs[0]'s model; n_inputs is needed when there is no weight
        matrix to read the input length from.
        total_const_size: the settings' count of constant cells (None: 4 as ever; with Fixed parameters what a dummy pass would count:
        one cell per distinct value among the parameters and the layout's own constants, `_own_constants`)"""
        self.k, self.w = logrows, num_inner_cols
        self.weights = [[[int(v) for v in row] for row in W] for W in weights]
        self.biases = [[int(v) for v in b] for b in biases]
        self.base, self.legs, self.relu_last, self.relu_first = decomp_base, decomp_legs, relu_last, bool(relu_first)
        self.rebase = [1] * len(self.weights) if rebase is None else [int(d) for d in rebase]
        if len(self.rebase) != len(self.weights) or any(not 1 <= d < 1 << 32 for d in self.rebase):
            raise ValueError("MlpCircuit: rebase takes one divisor in [1, 2^32) per layer")
        self.n_inputs = int(n_inputs) if n_inputs is not None else (len(self.weights[0][0]) if self.weights else None)
        if self.n_inputs is None or (self.weights and len(self.weights[0][0]) != self.n_inputs):
            raise ValueError("MlpCircuit: the input length is unknown or does not match the first weight matrix")
        self.visibility = visibility_triple(visibility)
        if total_assignments is None:                  # the dummy layout pass of gen-settings: count the cells
            total_assignments = self._count_cells()
        self.n_outputs = len(self.weights[-1]) if self.weights else self.n_inputs
        self.n_params = sum(len(W) * len(W[0]) + len(b) for W, b in zip(self.weights, self.biases))
        if total_const_size is None and self.visibility[1] == "Fixed":      # one constant cell per distinct value
            total_const_size = len(set(self._own_constants()) | {v % R for v in self.flat_params()})
        self._configure(total_assignments, 4 if total_const_size is None else int(total_const_size))

    def _own_constants(self):
        """the constants the layout itself places, whatever the parameters are -- zeros (the padding of a dot whose length is no multiple of
        the width, the equalities of equals_zero), ones, the powers of the decomposition base, what `div` needs of its divisor --, read off
        a dummy pass over a MINIATURE of this circuit: same options, same divisors, zero parameters that are Private, every dimension d
        beyond two rows cut to w + d % w (a constant's value never depends on a length, only a dot's padding on its residue).  Costs
        nothing next to a pass over the circuit itself, which every `verify` of a description with Fixed parameters would pay otherwise"""
        w = self.w
        cut = lambda d: d if d <= 2 * w else w + d % w
        dims = [cut(self.n_inputs)] + [cut(len(W)) for W in self.weights]
        mini = MlpCircuit(self.k, w, [[[0] * dims[i]] * dims[i + 1] for i in range(len(self.weights))], [[0] * d for d in dims[1:]], self.base, self.legs,
                          relu_last=self.relu_last, n_inputs=dims[0], relu_first=self.relu_first, rebase=self.rebase,
                          visibility=(self.visibility[0], "Private", self.visibility[2]))
        reg = BaseRegion(mini.gc, False)
        mini.layout(reg, [Val(0)] * dims[0], Val)
        return [v for v, _ in reg.const_order]

    def _configure(self, total_assignments, total_const_size):
        vin, vpar, vout = self.visibility
        # module_sizes.polycommit (src/graph/mod.rs:1344-1356, modules.rs:171-205): input, ALL parameters as one tensor, output; a tensor of
        # length 0 has no module
        sizes = [n for v, n in zip(self.visibility, (self.n_inputs, self.n_params, self.n_outputs)) if v == "KZGCommit" and n > 0]
        shapes = ([[1, self.n_inputs]] if vin == "Public" else []) + ([[1, self.n_outputs]] if vout == "Public" else [])
        # max_rows uses blinding factors = 5 (no gate queries 3+ rotations of a column)
        self.settings = EC.GraphSettings(self.k, self.w, total_assignments, total_const_size=total_const_size,
                                         required_range_checks=[(-1, 1), (0, self.base - 1)], model_instance_shapes=shapes,
                                         polycommit_sizes=sizes, always_instance=True)
        self.gc = EC.GraphConfig(self.settings)

    def flat_params(self):
        """every parameter in the order `layout` asks for them: what a KZGCommit of the parameters commits to"""
        return [v for W, b in zip(self.weights, self.biases) for v in [wv for row in W for wv in row] + list(b)]

    def _count_cells(self):
        w, lg = self.w, self.legs
        def dec(m): return _decomposition_cells(m, w, lg)
        def al(c): return -(-c // w) * w
        c = dec(self.n_inputs)
        if self.relu_first:
            c += dec(self.n_inputs) + 6 * self.n_inputs
        for i, W in enumerate(self.weights):
            m, kk = len(W), len(W[0])
            c = al(c) + m * al(kk) + m
            if self.rebase[i] != 1:                    # div: three decompositions (claim, |diff|, d - |diff|) and 16 cells of pairwise / equality ops
                c += 3 * (dec(m) + w) + 16 * m
            if i + 1 < len(self.weights) or self.relu_last:
                c += dec(m) + 6 * m
        m = len(self.weights[-1]) if self.weights else self.n_inputs
        return c + 2 * dec(m) + m + 64

    def _modules(self):
        """the PolyCommit column set of the input, the parameters and the output (None: the tensor is not committed)"""
        it = iter(self.gc.polycommit)
        return [next(it) if v == "KZGCommit" and n > 0 else None
                for v, n in zip(self.visibility, (self.n_inputs, self.n_params, self.n_outputs))]

    def committed(self):
        """[(tensor name, its module's VarTensor, its length)] of the KZG-committed tensors, in the order of their columns"""
        lengths = (self.n_inputs, self.n_params, self.n_outputs)
        return [(what, var, n) for what, var, n in zip(("input", "params", "output"), self._modules(), lengths) if var is not None]

    def layout(self, reg, inputs, param):
        """the op sequence, stated once: `synthesize` runs it on a BaseRegion with the input's values, witness_plan.record_plan on a
        recording region with symbols.  inputs: the input vector as Vals; param(v) -> the Val of a circuit parameter (they are asked for
        in a fixed order: per layer, each weight row, then the biases).  Around the model, in the order of GraphCircuit::synthesize:
        the input's module, the parameters' module, the model, the output's module (PolyCommitChip::layout: VarTensor::assign from row 0)."""
        reg.decomp = (self.base, self.legs)
        vin, vpar, vout = self.visibility
        m_in, m_par, m_out = self._modules()
        inst = self.gc.instance
        if m_in is not None:
            inputs = reg.assign(m_in, inputs, 0)
        elif vin == "Public":                          # the model's first use of a ValTensor::Instance: assign_advice_from_instance, without advancing
            inputs = reg.assign(reg.inputs[0], [Val(v.v, ("inst", inst.index, t)) for t, v in enumerate(inputs)])
        if m_par is not None:                          # one module for all parameters; the model reads its cells (replace_consts)
            committed = iter(reg.assign(m_par, [param(v) for v in self.flat_params()], 0))
            param = lambda v: next(committed)
        elif vpar == "Fixed":
            param = lambda v: Val(int(v), const=True)
        _, vals = reg.decompose(inputs, self.base, self.legs)                   # input range check
        if self.relu_first:
            vals = reg.relu(vals, self.base, self.legs)
        for i, (W, b) in enumerate(zip(self.weights, self.biases)):
            outs = [reg.dot(vals, [param(wv) for wv in row]) for row in W]         # einsum_with_base_ops: one dot per output
            outs = reg.div(outs, self.rebase[i])                                   # RebaseScale around the Einsum node
            vals = reg.pairwise(outs, [param(bv) for bv in b], EC.ADD)
            if i + 1 < len(self.weights) or self.relu_last:
                vals = reg.relu(vals, self.base, self.legs)
        if vout == "Public":
            reg.output_equals_instance(vals, inst, self.n_inputs if vin == "Public" else 0, self.base, self.legs)
        elif m_out is not None:                        # copy_advice of every output into the module's column: no `output` op
            reg.assign(m_out, vals, 0)
        return vals                                                              # the values the final equality is made on

    def plan_identity(self):
        """what a witness plan of this circuit depends on besides the layout code (witness_plan.params_hash)"""
        shape = [self.k, self.w, self.base, self.legs, int(self.relu_last), int(self.relu_first), self.n_inputs, len(self.weights)]
        per_layer = [a for W, b in zip(self.weights, self.biases) for a in ([len(W), len(W[0]), len(b)], W, b)]
        rebase = [self.rebase] if any(d != 1 for d in self.rebase) else []      # (a circuit that rescales nothing keeps its hash)
        ident = b"".join(np.asarray(a, np.int64).tobytes() for a in [shape] + per_layer + rebase)
        if self.visibility != DEFAULT_VISIBILITY:      # (the default triple keeps its hash)
            ident += ("visibility:%s/%s/%s" % self.visibility).encode()
        return ident

    def config(self):
        return dict(logrows=self.k, num_inner_cols=self.w, weights=self.weights, biases=self.biases, decomp_base=self.base, decomp_legs=self.legs,
                    total_assignments=self.settings.total_assignments, relu_last=self.relu_last, n_inputs=self.n_inputs,
                    relu_first=self.relu_first, rebase=self.rebase, visibility=self.visibility, total_const_size=self.settings.total_const_size)

    def synthesize(self, x, witness=True):
        reg = super().synthesize(x, witness)
        self.public = self.instances(x)[0]
        return reg

    def instances(self, x, outputs=None):
        """the instance column of a witness (prepare_public_inputs): the input where it is public, then the output where it is;
        outputs: None = those of the last synthesis"""
        outputs = self.outputs if outputs is None else outputs
        return [([int(v) % R for v in x] if self.visibility[0] == "Public" else []) +
                ([int(v) % R for v in outputs] if self.visibility[2] == "Public" else [])]

    def witness_of(self, reg):
        n = 1 << self.k
        return [reg.advice.get(c.index) or [0] * n for c in self.gc.cs.advice], [self.public]


def _given_parameters(circuit, **arrays):
    """the parameter arrays a caller hands a circuit in place of its seeded ones (None: keep the seeded one): int64 integers in the shape
    the seeded array has; anything else is a ValueError that names the array"""
    for name, given in arrays.items():
        if given is None:
            continue
        want = getattr(circuit, name).shape
        try:
            a = np.array(given, dtype=object)
        except ValueError:
            a = None
        if a is None or a.shape != want:
            raise ValueError("%s: the circuit takes an array of shape %s" % (name, list(want)))
        flat = a.reshape(-1).tolist()
        if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not -(1 << 63) <= int(v) < 1 << 63 for v in flat):
            raise ValueError("%s: every entry is an integer that fits int64" % name)
        setattr(circuit, name, np.array([int(v) for v in flat], np.int64).reshape(want))


class ConvMnistConfig(EC.GraphConfig):
    """the Config of /root/reference/examples/conv2d_mnist/main.rs:148-186, in its order: three one-column advice VarTensors (input,
    params, output), the constant columns, BaseConfig over them, range checks (-1, 1) and (0, base - 1) (RegionCtx's decomposition:
    base 1024, 2 legs), the Div{denom} static lookup over (lookup_min, lookup_max), then the public-output instance column"""

    def __init__(self, logrows, length, lookup_range, denom, decomp_base=1024, num_inner_cols=1, capacity=None):
        cs = self.cs = EC.ConstraintSystem()
        length = capacity or length                    # the example sizes its VarTensors by LEN (one column each); tests may ask for more blocks
        self.settings = EC.GraphSettings(logrows, num_inner_cols, length, total_const_size=length,
                                         required_range_checks=[(-1, 1), (0, decomp_base - 1)], model_instance_shapes=[[1, 10]])
        self.advices = [EC.VarTensor.new_advice(cs, logrows, num_inner_cols, length) for _ in range(3)]
        self.const_cols = EC.VarTensor.constant_cols(cs, logrows, length)
        inp, params, out = self.advices
        base = self.base = EC.BaseConfig(cs, [inp, params], out)
        base.configure_range_check(inp, params, (-1, 1), logrows)
        base.configure_range_check(inp, params, (0, decomp_base - 1), logrows)
        self.div = lambda x: round_div(x, denom)
        base.configure_lookup(inp, out, params, tuple(lookup_range), logrows, "div_%d" % denom, self.div)
        self.instance = cs.instance_column()
        cs.enable_equality(self.instance)
        cs.chunk_lookups()


class ConvMnistCircuit(LayoutCircuit):
    """examples/conv2d_mnist (BASELINE configs[2]): Conv 1 -> 4 channels, 5 x 5, stride 2 over a 28 x 28 image (one dot product of
    25 + a bias addition per output, layouts.rs:4499-4661), LeakyReLU slope 0 (sign by decomposition), Div{32} through a static
    lookup table over (-32768, 32768) -- 65 537 rows: this is what makes the circuit k = 17 --, a 576 -> 10 linear layer
    ("ij,j->ik" = 10 dot products of 576, layouts.rs:887-1098) and its bias; the 10 outputs are tied to the instance column.
    The example reads MNIST and trained parameters from files that are not in the repository; shapes and value ranges are what
    matter to the prover, the data is synthetic."""

    def __init__(self, logrows=17, image=28, kernel=5, out_channels=4, stride=2, classes=10, lookup_range=(-32768, 32768), denom=32,
                 decomp_base=1024, decomp_legs=2, seed=0, num_inner_cols=1, capacity=None, kernels=None, conv_bias=None, fc_w=None, fc_b=None):
        """kernels [oc][K][K], conv_bias [oc], fc_w [classes][oc * slides^2], fc_b [classes]: the parameters as integers (a shape that
        does not fit is a ValueError naming the array); an array that is absent keeps its seeded synthetic values"""
        self.k, self.w = logrows, num_inner_cols
        self.image, self.kernel, self.oc, self.stride, self.classes = image, kernel, out_channels, stride, classes
        self.slides = (image - kernel) // stride + 1
        self.n_inputs = image * image
        self.length = out_channels * self.slides * self.slides
        self.base, self.legs, self.denom = decomp_base, decomp_legs, denom
        self.lookup_range, self.seed, self.capacity = tuple(lookup_range), seed, capacity
        rng = np.random.default_rng(seed)
        self.kernels = rng.integers(-20, 21, (out_channels, kernel, kernel))               # round(32 * trained float), main.rs:346-358
        self.conv_bias = np.zeros(out_channels, np.int64)                                 # main.rs:366-367
        self.fc_w = rng.integers(-12, 13, (classes, self.length))
        self.fc_b = rng.integers(-40, 41, classes)
        _given_parameters(self, kernels=kernels, conv_bias=conv_bias, fc_w=fc_w, fc_b=fc_b)
        self.gc = ConvMnistConfig(logrows, self.length, lookup_range, denom, decomp_base, num_inner_cols, capacity)

    def config(self):
        return dict(logrows=self.k, image=self.image, kernel=self.kernel, out_channels=self.oc, stride=self.stride, classes=self.classes,
                    lookup_range=self.lookup_range, denom=self.denom, decomp_base=self.base, decomp_legs=self.legs, seed=self.seed,
                    num_inner_cols=self.w, capacity=self.capacity, kernels=self.kernels, conv_bias=self.conv_bias, fc_w=self.fc_w, fc_b=self.fc_b)

    def model(self, img):
        """the integer forward pass the circuit proves"""
        img = np.asarray(img, np.int64).reshape(self.image, self.image)
        s, K = self.slides, self.kernel
        conv = np.array([[[int((img[i * self.stride:i * self.stride + K, j * self.stride:j * self.stride + K] * self.kernels[o]).sum()) + int(self.conv_bias[o])
                           for j in range(s)] for i in range(s)] for o in range(self.oc)]).reshape(-1)
        act = np.array([self.gc.div(max(int(v), 0)) for v in conv])
        return [int(v) for v in self.fc_w @ act + self.fc_b]

    def layout(self, reg, inputs, param):
        """the op sequence, stated once: `synthesize` runs it on a BaseRegion with the image's values, witness_plan.record_plan on a
        recording region with symbols.  inputs: the image, row-major, as Vals; param(v) -> the Val of a circuit parameter (they are
        asked for in a fixed order: kernels, then per output its conv bias, the linear layer's rows, its biases)"""
        vals = reg.conv([param(v) for v in self.kernels.reshape(-1)], inputs, lambda o: param(self.conv_bias[o]), self.oc, self.image, self.kernel, self.stride)
        vals = reg.relu(vals, self.base, self.legs)
        vals = reg.nonlinearity(vals, "div_%d" % self.denom)
        outs = [reg.dot([param(v) for v in row], vals) for row in self.fc_w]
        outs = reg.pairwise(outs, [param(v) for v in self.fc_b], EC.ADD)
        reg.constrain_instance(outs, self.gc.instance)
        return outs

    def plan_identity(self):
        """what a witness plan of this circuit depends on besides the layout code and the lookup tables (witness_plan.params_hash)"""
        shape = [self.k, self.w, self.image, self.kernel, self.oc, self.stride, self.classes, self.base, self.legs, self.denom,
                 self.gc.advices[0].num_blocks()]
        return b"".join(np.asarray(a, np.int64).tobytes() for a in (shape, self.kernels, self.conv_bias, self.fc_w, self.fc_b))


class SumProdCircuit(LayoutCircuit):
    """the accumulated SUM / CUMPROD gates of BaseConfig (chip.rs:343-359, base.rs) on a private vector: instance = [sum(x), prod(x),
    sum of the pairwise products x_i * x_{i+1}] -- used by the tests that drive the gates the MLP / conv circuits never switch on"""

    def __init__(self, logrows, num_inner_cols, capacity):
        self.k, self.w, self.capacity = logrows, num_inner_cols, capacity
        self.settings = EC.GraphSettings(logrows, num_inner_cols, capacity, total_const_size=4, required_range_checks=[], model_instance_shapes=[[1, 3]])
        self.gc = EC.GraphConfig(self.settings)

    def config(self):
        return dict(logrows=self.k, num_inner_cols=self.w, capacity=self.capacity)

    def synthesize(self, x, witness=True):
        reg = BaseRegion(self.gc, witness)
        vals = reg.assign(reg.inputs[0], [Val(int(v) % R) for v in x])
        reg.increment(len(vals))
        s = reg.sum(vals)
        p = reg.prod(vals)
        pw = reg.pairwise(vals[:-1], vals[1:], EC.MULT)
        sp = reg.sum(pw)
        outs = [s, p, sp]
        reg.constrain_instance(outs, self.gc.instance)
        reg.finish(self.gc.const_cols)
        self.outputs = [v.v for v in outs]
        return reg


class SumProdLayoutCircuit(SumProdCircuit):
    """SumProdCircuit with its op sequence stated once (`layout`), so that witness_plan.record_plan can run it on symbols: the same
    cells, values, selectors and copies as its parent's `synthesize`.  length: the number of inputs."""
    synthesize = LayoutCircuit.synthesize              # (not the parent's: that one states the ops a second time)

    def __init__(self, logrows, num_inner_cols, capacity, length):
        super().__init__(logrows, num_inner_cols, capacity)
        self.n_inputs = int(length)

    def config(self):
        return dict(super().config(), length=self.n_inputs)

    def layout(self, reg, inputs, param):
        vals = reg.assign(reg.inputs[0], inputs)
        reg.increment(len(vals))
        s = reg.sum(vals)
        p = reg.prod(vals)
        pw = reg.pairwise(vals[:-1], vals[1:], EC.MULT)
        sp = reg.sum(pw)
        outs = [s, p, sp]
        reg.constrain_instance(outs, self.gc.instance)
        return outs

    def plan_identity(self):
        return np.asarray([self.k, self.w, self.n_inputs, self.gc.advices[0].num_blocks()], np.int64).tobytes()


class SortTopkCircuit(LayoutCircuit):
    """a top-k and a full sort of one private vector (layouts.rs `topk_axes` / `_sort_ascending`): instance = the k_top largest (or
    smallest) values, then the whole vector in ascending order under `mode`.  The op sequence is stated once (`layout`), so that
    witness_plan.record_plan can run it on symbols.  The settings carry the range checks of the decomposition, (-1, 1) and (0, base - 1),
    the (0, 1) check of `and` / `or` in the indexed modes, and the shuffle argument."""

    def __init__(self, logrows, num_inner_cols, capacity, length, k_top, largest=True, mode="unsorted", decomp_base=16, decomp_legs=2):
        assert mode in SORT_MODES and 1 <= k_top <= length
        self.k, self.w, self.capacity, self.n_inputs = logrows, num_inner_cols, capacity, int(length)
        self.k_top, self.largest, self.mode, self.base, self.legs = int(k_top), bool(largest), mode, decomp_base, decomp_legs
        checks = [(-1, 1), (0, decomp_base - 1)] + ([(0, 1)] if mode != "unsorted" else [])
        self.settings = EC.GraphSettings(logrows, num_inner_cols, capacity, total_const_size=4, required_range_checks=checks,
                                         model_instance_shapes=[[1, self.k_top + self.n_inputs]], total_shuffle_col_size=2 * self.n_inputs,
                                         num_shuffles=1)
        self.gc = EC.GraphConfig(self.settings)

    def layout(self, reg, inputs, param):
        reg.decomp = (self.base, self.legs)
        vals = reg.assign(reg.inputs[0], inputs)
        reg.increment(len(vals))
        top = reg.topk(vals, self.k_top, self.largest)
        srt, _ = reg.sort_ascending(vals, self.mode)
        outs = top + srt
        reg.constrain_instance(outs, self.gc.instance)
        return outs

    def plan_identity(self):
        shape = [self.k, self.w, self.n_inputs, self.k_top, int(self.largest), SORT_MODES.index(self.mode), self.base, self.legs, self.gc.advices[0].num_blocks()]
        return np.asarray(shape, np.int64).tobytes()

    def config(self):
        return dict(logrows=self.k, num_inner_cols=self.w, capacity=self.capacity, length=self.n_inputs, k_top=self.k_top, largest=self.largest,
                    mode=self.mode, decomp_base=self.base, decomp_legs=self.legs)


class NormCircuit(LayoutCircuit):
    """the two normalisations of a transformer on `rows` x `length` private inputs, instance = the outputs, row by row.  Softmax
    (layouts.rs `softmax_axes` along the rows): max by an `unsorted` sort, the exp table, sum, the claimed reciprocal, MULT -- outputs at
    input_scale * output_scale.  With layer_norm: x - mean (`sum`, `div`), `mean_of_squares`, `rsqrt` (the claimed root, then the claimed
    reciprocal), MULT, `div` by the input scale -- outputs at the output scale.  The op sequence is stated once (`layout`), so that
    witness_plan.record_plan can run it on symbols.  The settings carry the range checks of the decomposition, (-1, 1) and (0, base - 1),
    the (0, 1) check of `and` / `iff`, and for the softmax the shuffle argument of the sort and the exp table over `lookup_range`.  eps:
    what `recip` adds to a zero input (zero_inverse = round(output_scale / eps) must fit the decomposition, as every |claim * x - S| must)."""

    def __init__(self, logrows, num_inner_cols, capacity, rows, length, input_scale=8, output_scale=64, eps=1.0 / 128, layer_norm=False,
                 decomp_base=128, decomp_legs=2, lookup_range=(-255, 0)):
        self.k, self.w, self.rows, self.length, self.n_inputs = logrows, num_inner_cols, int(rows), int(length), int(rows) * int(length)
        self.capacity = capacity
        self.input_scale, self.output_scale, self.eps, self.layer_norm = int(input_scale), int(output_scale), float(eps), bool(layer_norm)
        self.base, self.legs, self.lookup_range = decomp_base, decomp_legs, tuple(lookup_range)
        assert self.input_scale >= 1 and self.output_scale >= 1 and abs(zero_recip(self.output_scale, self.eps)) < decomp_base ** decomp_legs
        scale = self.input_scale
        self.exp = lambda x: int(math.floor(scale * math.exp(x / scale) + 0.5))         # LookupOp::Exp { scale, base: e } (ops.rs `exp`)
        softmax = dict(required_lookups=[("exp", self.exp)], lookup_range=self.lookup_range, total_shuffle_col_size=self.n_inputs, num_shuffles=1)
        self.settings = EC.GraphSettings(logrows, num_inner_cols, capacity, total_const_size=8, required_range_checks=[(-1, 1), (0, decomp_base - 1), (0, 1)],
                                         model_instance_shapes=[[self.rows, self.length]], **({} if self.layer_norm else softmax))
        self.gc = EC.GraphConfig(self.settings)

    def layout(self, reg, inputs, param):
        reg.decomp = (self.base, self.legs)
        L, si, so, eps = self.length, self.input_scale, self.output_scale, self.eps
        vals = reg.assign(reg.inputs[0], inputs)
        reg.increment(len(vals))
        rows = [vals[i * L:(i + 1) * L] for i in range(self.rows)]
        if self.layer_norm:
            means = reg.div([reg.sum(row) for row in rows], L)
            centred = [reg.pairwise(row, [mean] * L, EC.SUB) for row, mean in zip(rows, means)]
            inv = reg.rsqrt(reg.mean_of_squares(centred), si, so, eps)
            outs = [v for row, r in zip(centred, inv) for v in reg.div(reg.pairwise(row, [r] * L, EC.MULT), si)]
        else:
            outs = [v for row in reg.softmax_axes(rows, si, so, eps) for v in row]
        reg.constrain_instance(outs, self.gc.instance)
        return outs

    def plan_identity(self):
        shape = [self.k, self.w, self.rows, self.length, self.input_scale, self.output_scale, int(self.layer_norm), self.base, self.legs,
                 self.lookup_range[0], self.lookup_range[1], self.gc.advices[0].num_blocks()]
        return np.asarray(shape, np.int64).tobytes() + np.float64(self.eps).tobytes()

    def config(self):
        return dict(logrows=self.k, num_inner_cols=self.w, rows=self.rows, length=self.length, input_scale=self.input_scale,
                    output_scale=self.output_scale, eps=self.eps, layer_norm=self.layer_norm, decomp_base=self.base, decomp_legs=self.legs,
                    lookup_range=self.lookup_range, capacity=self.capacity)


class PoolClassifierCircuit(LayoutCircuit):
    """a LeNet-shaped classifier on a private `image` x `image` picture: a convolution with bias (one `dot` per output and a bias addition,
    as ConvMnistCircuit lays it out), `relu`, a pooling layer -- pool = "max": `max_pool`, "sum": `sumpool`, normalized --, a linear layer
    with bias and `argmax` of its logits; instance = the logits, then the class index.  The op sequence is stated once (`layout`), so that
    witness_plan.record_plan can run it on symbols.  The settings carry the range checks of the decomposition, (-1, 1) and (0, base - 1),
    the (0, 1) check of the indexed sort of `argmax`, the shuffle argument of the sorts and the dynamic lookup of `select`.  Parameters
    are seeded synthetic integers, as ConvMnistCircuit's are."""

    def __init__(self, logrows, num_inner_cols, capacity, image=8, kernel=3, out_channels=2, stride=1, pool_size=2, pool_stride=2, classes=4,
                 pool="max", decomp_base=128, decomp_legs=3, seed=0, kernels=None, conv_bias=None, fc_w=None, fc_b=None):
        """kernels [oc][K][K], conv_bias [oc], fc_w [classes][oc * pooled^2], fc_b [classes]: the parameters as integers (a shape that
        does not fit is a ValueError naming the array); an array that is absent keeps its seeded synthetic values"""
        assert pool in ("max", "sum"), pool
        self.k, self.w, self.capacity = logrows, num_inner_cols, capacity
        self.image, self.kernel, self.oc, self.stride, self.classes = image, kernel, out_channels, stride, classes
        self.pool, self.pool_size, self.pool_stride, self.seed = pool, pool_size, pool_stride, seed
        self.base, self.legs = decomp_base, decomp_legs
        self.slides = (image - kernel) // stride + 1
        self.pooled = (self.slides - pool_size) // pool_stride + 1
        self.n_inputs = image * image
        self.length = out_channels * self.pooled * self.pooled
        rng = np.random.default_rng(seed)
        self.kernels = rng.integers(-4, 5, (out_channels, kernel, kernel))
        self.conv_bias = rng.integers(-8, 9, out_channels)
        self.fc_w = rng.integers(-4, 5, (classes, self.length))
        self.fc_b = rng.integers(-16, 17, classes)
        _given_parameters(self, kernels=kernels, conv_bias=conv_bias, fc_w=fc_w, fc_b=fc_b)
        windows = self.length if pool == "max" and pool_size > 1 else 0        # one sort per window; a `max` of one element sorts nothing
        sort_rows = windows * pool_size * pool_size + (classes if classes > 1 else 0)
        self.settings = EC.GraphSettings(logrows, num_inner_cols, capacity, total_const_size=16, required_range_checks=[(-1, 1), (0, decomp_base - 1), (0, 1)],
                                         model_instance_shapes=[[1, classes + 1]], total_dynamic_col_size=classes, num_dynamic_lookups=1,
                                         total_shuffle_col_size=max(sort_rows, 1), num_shuffles=windows + 1)
        self.gc = EC.GraphConfig(self.settings)

    def model(self, img):
        """the integer forward pass the circuit proves: the logits, then the first index of their maximum"""
        img = np.asarray(img, np.int64).reshape(self.image, self.image)
        s, K, st, q, P, ps = self.slides, self.kernel, self.stride, self.pooled, self.pool_size, self.pool_stride
        conv = np.array([[[max(int((img[i * st:i * st + K, j * st:j * st + K] * self.kernels[o]).sum()) + int(self.conv_bias[o]), 0)
                           for j in range(s)] for i in range(s)] for o in range(self.oc)])
        win = lambda o, i, j: conv[o, i * ps:i * ps + P, j * ps:j * ps + P]
        if self.pool == "max":
            act = [int(win(o, i, j).max()) for o in range(self.oc) for i in range(q) for j in range(q)]
        else:
            act = [round_div(int(win(o, i, j).sum()), P * P) for o in range(self.oc) for i in range(q) for j in range(q)]
        logits = [int(v) for v in self.fc_w @ np.array(act, np.int64) + self.fc_b]
        return logits + [max(range(len(logits)), key=lambda j: (logits[j], -j))]

    def layout(self, reg, inputs, param):
        """inputs: the image, row-major, as Vals; param(v) -> the Val of a circuit parameter (asked for in a fixed order: kernels, then per
        output its conv bias, the linear layer's rows, its biases)"""
        reg.decomp = (self.base, self.legs)
        s = self.slides
        vals = reg.conv([param(v) for v in self.kernels.reshape(-1)], inputs, lambda o: param(self.conv_bias[o]), self.oc, self.image, self.kernel, self.stride)
        vals = reg.relu(vals, self.base, self.legs)
        geometry = (self.oc, s, s, ((0, 0), (0, 0)), (self.pool_stride,) * 2, (self.pool_size,) * 2)
        vals = reg.max_pool(vals, *geometry) if self.pool == "max" else reg.sumpool(vals, *geometry, True)
        logits = [reg.dot([param(v) for v in row], vals) for row in self.fc_w]
        logits = reg.pairwise(logits, [param(v) for v in self.fc_b], EC.ADD)
        outs = logits + [reg.argmax(logits)]
        reg.constrain_instance(outs, self.gc.instance)
        return outs

    def plan_identity(self):
        shape = [self.k, self.w, self.image, self.kernel, self.oc, self.stride, self.pool_size, self.pool_stride, self.classes,
                 int(self.pool == "max"), self.base, self.legs, self.gc.advices[0].num_blocks()]
        return b"".join(np.asarray(a, np.int64).tobytes() for a in (shape, self.kernels, self.conv_bias, self.fc_w, self.fc_b))

    def config(self):
        return dict(logrows=self.k, num_inner_cols=self.w, image=self.image, kernel=self.kernel, out_channels=self.oc, stride=self.stride,
                    pool_size=self.pool_size, pool_stride=self.pool_stride, classes=self.classes, pool=self.pool, decomp_base=self.base,
                    decomp_legs=self.legs, seed=self.seed, capacity=self.capacity, kernels=self.kernels, conv_bias=self.conv_bias, fc_w=self.fc_w,
                    fc_b=self.fc_b)


class ScatterGatherCircuit(LayoutCircuit):
    """a table update and two lookups on private inputs -- a `rows` x `cols` table, an `m` x `cols` index, an `m` x `cols` source and `p`
    row picks, in that order, each row-major: t = `scatter_elements`(table, index, src) along dim 0 (x[idx] = v, a cache update), g =
    `gather`(t, picks) along dim 0 (an embedding lookup) and h = `one_hot`(picks[0], rows) (a label); instance = g, then h.  The op
    sequence is stated once (`layout`), so that witness_plan.record_plan can run it on symbols.  For a satisfiable witness every COLUMN of
    the index must hold distinct values in [0, rows): two elements on one target leave the permutation argument of the missing set without
    a witness.  The settings carry the range checks of the decomposition, (-1, 1) and (0, base - 1), the (0, 1) check of `one_hot`, the
    dynamic lookups of the gathers and the shuffle arguments of the missing set and its sort (base^legs must exceed rows * cols)."""

    def __init__(self, logrows, num_inner_cols, capacity, rows=6, cols=3, m=2, picks=4, decomp_base=128, decomp_legs=2):
        assert 1 <= m <= rows and cols >= 1 and picks >= 1 and decomp_base ** decomp_legs > rows * cols
        self.k, self.w, self.capacity = logrows, num_inner_cols, capacity
        self.rows, self.cols, self.m, self.picks, self.base, self.legs = int(rows), int(cols), int(m), int(picks), decomp_base, decomp_legs
        n = self.rows * self.cols
        self.n_inputs = n + 2 * self.m * self.cols + self.picks
        self.settings = EC.GraphSettings(logrows, num_inner_cols, capacity, total_const_size=16, required_range_checks=[(-1, 1), (0, decomp_base - 1), (0, 1)],
                                         model_instance_shapes=[[1, self.picks * self.cols + self.rows]], total_dynamic_col_size=4 * n + self.rows,
                                         num_dynamic_lookups=5, total_shuffle_col_size=2 * n - self.m * self.cols, num_shuffles=2)
        self.gc = EC.GraphConfig(self.settings)

    def _split(self, x):
        n, mc = self.rows * self.cols, self.m * self.cols
        return x[:n], x[n:n + mc], x[n + mc:n + 2 * mc], x[n + 2 * mc:]

    def model(self, x):
        """the integer forward pass the circuit proves: the gathered rows of the updated table, then the one-hot vector of the first pick"""
        table, index, src, picks = (np.asarray(a, np.int64) for a in self._split(list(x)))
        t = table.reshape(self.rows, self.cols).copy()
        np.put_along_axis(t, index.reshape(self.m, self.cols), src.reshape(self.m, self.cols), axis=0)
        return [int(v) for v in np.take(t, picks, axis=0).reshape(-1)] + [int(j == picks[0]) for j in range(self.rows)]

    def layout(self, reg, inputs, param):
        reg.decomp = (self.base, self.legs)
        vals = reg.assign(reg.inputs[0], inputs)
        reg.increment(len(vals))
        table, index, src, picks = self._split(vals)
        t = reg.scatter_elements(table, [self.rows, self.cols], index, [self.m, self.cols], src, 0)
        g = reg.gather(t, [self.rows, self.cols], picks, 0)
        h = reg.one_hot(picks[0], self.rows)
        outs = g + h
        reg.constrain_instance(outs, self.gc.instance)
        return outs

    def plan_identity(self):
        shape = [self.k, self.w, self.rows, self.cols, self.m, self.picks, self.base, self.legs, self.gc.advices[0].num_blocks()]
        return np.asarray(shape, np.int64).tobytes()

    def config(self):
        return dict(logrows=self.k, num_inner_cols=self.w, capacity=self.capacity, rows=self.rows, cols=self.cols, m=self.m, picks=self.picks,
                    decomp_base=self.base, decomp_legs=self.legs)


class _CopyArray:
    """copy constraints as the (count, 4) uint32 array the native keygen takes (native._copies_array reads `.array`); iterable as pairs
    for the Python keygen of small circuits"""

    def __init__(self, array):
        self.array = np.ascontiguousarray(array, np.uint32).reshape(-1, 4)

    def __len__(self):
        return self.array.shape[0]

    def __iter__(self):
        for a, b, c, d in self.array.tolist():
            yield (a, b), (c, d)


class TransformerSurrogateCircuit:
    """A SURROGATE for BASELINE configs[4] (examples/onnx/nanoGPT at k = 22, /root/reference/tests/integration_tests.rs:172-181) that
    switches on the argument families a transformer circuit switches on and the MLP surrogate does not -- NOT the nanoGPT graph (its
    layout is ezkl's Model::layout, 6.8k lines of Rust: SURVEY.md §2 #5, out of scope):
      * the base gates over three model VarTensors (dot, sum, pairwise, decomposition range checks) -- attention scores, an MLP;
      * THREE static lookup tables over (-32768, 32768) (exp and reciprocal for a softmax, rsqrt for a layer norm:
        BaseConfig::configure_lookup, chip.rs:452-615), one mv-lookup argument per (table, block, inner column);
      * a DYNAMIC lookup (an embedding gather) and a SHUFFLE (a transpose), whose table side is advice x selector (chip.rs:619-833);
      * an einsum contraction with Freivalds RLC gates: SECOND-PHASE advice columns and two challenges (chip/einsum/mod.rs:487-783).
    One UNIT -- all of the above on a vector of d values and an L x L matmul -- is laid out by the layout engine on the real
    configuration; the unit is then repeated down every column and in every block with numpy (gates are row-local, copy constraints
    move with their tile, the lookup arguments are multiset statements over all rows), so the circuit is FULL (every tile is a valid
    witness of the same statement) without minutes of Python per cell and without a laid-out circuit in the repository.  Only the first
    tile's outputs are tied to the instance column."""
    lays_einsums = True                                # (what witness_plan asks of a class: see LayoutCircuit)

    def __init__(self, logrows, blocks=4, num_inner_cols=1, d=16, einsum_len=16, decomp_base=16384, decomp_legs=2, lookup_max=None, seed=1):
        import math
        assert num_inner_cols == 1, "the Freivalds layout here is the reference bench's: one inner column"
        self.k, self.w, self.d, self.L = logrows, num_inner_cols, d, einsum_len
        self.base, self.legs = decomp_base, decomp_legs
        n = 1 << logrows
        lm = self.lookup_max = lookup_max or min(32768, n // 8)
        room = n - min(64, n // 8)                                                     # rows of a column that are certainly usable
        cap_model = int((blocks - 0.1) * num_inner_cols * room)
        self.tables = [("exp", lambda x: int(round(math.exp(min(x, 0) / (lm / 8.0)) * 256))),
                       ("recip", lambda x: int(round((lm * 16.0) / max(x, 1)))),
                       ("rsqrt", lambda x: int(round(256.0 / math.sqrt(max(x, 1)))))]
        self.settings = EC.GraphSettings(logrows, num_inner_cols, cap_model, total_const_size=64, required_range_checks=[(-1, 1), (0, decomp_base - 1)],
                                         required_lookups=self.tables, lookup_range=(-lm, lm), model_instance_shapes=[[1, d]],
                                         total_dynamic_col_size=room // 2, num_dynamic_lookups=1, total_shuffle_col_size=room // 2 - 2, num_shuffles=1,
                                         einsum_reduction_length=room, einsum_max_output_axes=2)
        self.gc = EC.GraphConfig(self.settings)
        assert self.gc.advices[0].num_blocks() == blocks and all(v.num_blocks() == 1 for v in self.gc.advices[3:6])
        self.blocks = blocks
        self.ein = EinsumMatmulCircuit.over(self.gc, einsum_len)
        rng = np.random.default_rng(seed)
        self.x = rng.integers(-9, 10, d).tolist()
        self.Wq = rng.integers(-3, 4, (d, d)).tolist()
        self.W2 = rng.integers(-3, 4, (d, d)).tolist()
        self.b2 = rng.integers(-5, 6, d).tolist()
        self.emb = [(i, int(rng.integers(-50, 50)), int(rng.integers(-50, 50))) for i in range(8)]          # (token, two embedding coordinates)
        self.tokens = rng.integers(0, 8, 2 * d).tolist()
        self.perm_rows = [(i, int(rng.integers(1, 99)), int(rng.integers(1, 99))) for i in range(8)]
        self.perm = rng.permutation(8).tolist()
        self.A = rng.integers(-8, 8, (einsum_len, einsum_len))
        self.B = rng.integers(-8, 8, (einsum_len, einsum_len))

    # ---- one unit ---------------------------------------------------------------------------------------------------------------------
    @property
    def n_inputs(self):
        """x (d), the tokens (2 d), A then B (L x L each, row-major): the input vector of `layout`, of `build` and of a witness plan"""
        return 3 * self.d + 2 * self.L * self.L

    def default_inputs(self):
        """the seeded vectors the circuit is built with when nothing else is given"""
        return [int(v) for v in list(self.x) + list(self.tokens) + list(np.asarray(self.A).reshape(-1)) + list(np.asarray(self.B).reshape(-1))]

    def _split(self, inputs):
        d, L = self.d, self.L
        assert len(inputs) == self.n_inputs, "the surrogate takes %d inputs" % self.n_inputs
        mat = lambda flat: [flat[i * L:(i + 1) * L] for i in range(L)]
        return inputs[:d], inputs[d:3 * d], mat(inputs[3 * d:3 * d + L * L]), mat(inputs[3 * d + L * L:])

    def layout(self, reg, inputs, param):
        """the unit, stated once: `build` runs it on a BaseRegion with the inputs' values, witness_plan.record_plan on a recording region
        with symbols.  inputs: `n_inputs` Vals; param(v) -> the Val of a circuit parameter (asked for in a fixed order: Wq, W2, b2, the
        embedding rows, perm_rows).  Returns the values tied to the instance column."""
        lm, d = self.lookup_max, self.d
        clamp = lambda v: Val(clamped(signed(v.v), -lm, lm))           # the surrogate's stand-in for a rescale: not copy-constrained
        xs, tokens, A, B = self._split(list(inputs))
        _, x = reg.decompose(xs, self.base, self.legs)                                        # input range check
        # attention scores -> softmax: exp lookup, sum, reciprocal lookup, scaling
        q = [reg.dot(x, [param(w_) for w_ in row]) for row in self.Wq]
        e = reg.nonlinearity([clamp(v) for v in q], "exp")
        tot = reg.sum(e)
        inv = reg.nonlinearity([clamp(tot)], "recip")
        reg.pairwise(e, [inv[0]] * d, EC.MULT)
        # layer norm: sum of squares, rsqrt lookup, scaling
        ss = reg.dot(x, x)
        rs = reg.nonlinearity([clamp(ss)], "rsqrt")
        reg.pairwise(x, [rs[0]] * d, EC.MULT)
        # MLP: Gemm + bias + ReLU (sign by decomposition)
        outs = [reg.dot(x, [param(w_) for w_ in row]) for row in self.W2]
        h = reg.pairwise(outs, [param(b) for b in self.b2], EC.ADD)
        h = reg.relu(h, self.base, self.legs)
        # embedding gather (dynamic lookup: the row a token's VALUE names) and a transpose (shuffle)
        emb = [tuple(param(v) for v in row) for row in self.emb]
        reg.dynamic_lookup(emb, [reg.row_at(emb, t) for t in tokens])
        perm_rows = [tuple(param(v) for v in row) for row in self.perm_rows]
        reg.shuffle(perm_rows, self.perm)
        # the Freivalds einsum over the second-phase columns, then the public outputs
        reg.einsum(self.ein, A, B)
        reg.output_equals_instance(h, self.gc.instance, 0, self.base, self.legs)
        return h

    def plan_identity(self):
        """what a witness plan of this circuit depends on besides the layout code and the lookup tables (witness_plan.params_hash)"""
        shape = [self.k, self.blocks, self.d, self.L, self.base, self.legs, self.lookup_max]
        return b"".join(np.asarray(a, np.int64).tobytes() for a in (shape, self.perm, self.Wq, self.W2, self.b2, self.emb, self.perm_rows))

    def _einsum(self, reg, challenges, A, B):
        return self.ein.synthesize(A, B, challenges, region=reg)

    # ---- the tiling --------------------------------------------------------------------------------------------------------------------
    def _geometry(self, reg):
        gc, w = self.gc, self.w
        assert reg.linear < gc.advices[0].block_size(), "the unit must fit one block"
        rows = max(-(-reg.linear // w), getattr(reg, "dyn", 0), reg.coord) + 1
        return rows, reg.usable // rows

    def build(self, gpu=None, tiles=None, as_ints=False, inputs=None, synthesis="host"):
        """-> dict(cs, fixed, copies, advice (callable(phase, challenges) -> {column: Montgomery array}), instances, info): the inputs of
        keygen and create_proof.  tiles: repeat the unit this many times down the rows (default: as many as fit).  as_ints: the advice
        callback returns lists of canonical ints (the MockProver's input) instead of Montgomery arrays.  inputs: the `n_inputs` integers
        of the unit (default: the seeded vectors).  synthesis: "host" -- the unit laid out in Python, tiled with numpy, converted and
        uploaded per phase -- or "device" (needs gpu = ezkl_amd.backend): both phases and the tiling run on the device from the circuit's
        witness plan; `advice` then returns {column: DeviceBuffer} of one resident set of columns, `device_columns` names them for
        native.create_proof(..., device_columns=...), `witness` holds what to free (`free()`), and the instance vector comes from the
        plan's outputs."""
        _check_synthesis(synthesis, gpu, as_ints)
        gc, cs0, n = self.gc, self.gc.cs, 1 << self.k
        inputs = self.default_inputs() if inputs is None else [int(v) for v in inputs]
        reg = BaseRegion(gc, True)
        h = self.layout(reg, [Val(v) for v in inputs], Val)
        reg.finish(gc.const_cols)
        _, _, A_in, B_in = self._split(inputs)
        A_in, B_in = np.array(A_in, np.int64), np.array(B_in, np.int64)
        U, T = self._geometry(reg)
        if tiles is not None:
            T = min(T, tiles)
        B = self.blocks
        # columns and selectors that exist per block (the model VarTensors and everything keyed by (block, inner column))
        colmap = {}                                                             # block-0 advice column -> [column in block b]
        for v in gc.advices[0:3]:
            for y in range(self.w):
                colmap[v.inner[0][y].index] = [v.inner[b][y].index for b in range(B)]
        selmap = {}
        def per_block(dct, rekey):
            for key, s0 in dct.items():
                blk = rekey(key, None)
                if blk == 0:
                    selmap[s0.index] = [dct[rekey(key, b)].index for b in range(B)]
        base = gc.base
        per_block(base.selectors, lambda k_, b: k_[1] if b is None else (k_[0], b, k_[2]))
        per_block(base.static_selectors, lambda k_, b: k_[1] if b is None else (k_[0], b, k_[2]))
        per_block(base.range_selectors, lambda k_, b: k_[1] if b is None else (k_[0], b, k_[2]))
        per_block(base.dynamic_lookup_selectors, lambda k_, b: k_[1][0] if b is None else (k_[0], (b, k_[1][1])))
        per_block(base.shuffle_input_selectors, lambda k_, b: k_[1][0] if b is None else (k_[0], (b, k_[1][1])))
        # selector activations, tiled
        acts = [None] * len(cs0.selectors)
        def tiled_rows(a):
            out = np.zeros(n, bool)
            out[:T * U] = np.tile(a[:U], T)
            return out
        for si, a in enumerate(reg.activations):
            if a is None or not a[:U].any():
                continue
            assert not a[U:].any()
            for sb in selmap.get(si, [si]):
                acts[sb] = tiled_rows(a)
        sel_cols = cs0.compress_selectors(acts)
        if n <= 1 << 12:
            sel_cols = [c.tolist() for c in sel_cols]
        cs = cs0.to_plonk(self.k)
        tabs = gc.table_columns()
        n_pre = cs.n_fixed - len(sel_cols)
        fixed = [tabs.get(c) or reg.fixed.get(c) or [0] * n for c in range(n_pre)] + list(sel_cols)
        # copy constraints, tiled: cells of per-block columns move with (block, tile), cells of the other advice columns with the tile,
        # constants stay, the instance column belongs to the first tile
        pos = {kc: i for i, kc in enumerate(cs.perm)}
        kinds = {"adv": 0, "fix": 1, "inst": 2}
        unit = np.array([[kinds[a[0]], a[1], a[2], kinds[b[0]], b[1], b[2]] for a, b in reg.copies], np.int64).reshape(-1, 6)
        has_inst = (unit[:, 0] == 2) | (unit[:, 3] == 2)
        first_tile, unit = unit, unit[~has_inst]
        lut = {b: np.arange(max(len(cs0.advice), 1), dtype=np.int64) for b in range(B)}
        for c0, cb in colmap.items():
            for b in range(B):
                lut[b][c0] = cb[b]
        perm_adv = np.full(len(cs0.advice), -1, np.int64)
        perm_fix = np.full(cs.n_fixed + 1, -1, np.int64)
        perm_inst = np.full(max(cs.n_instance, 1), -1, np.int64)
        for (kind, c), i in pos.items():
            (perm_adv if kind == "adv" else perm_fix if kind == "fix" else perm_inst)[c] = i
        per_blk = np.zeros(len(cs0.advice), bool)
        per_blk[list(colmap)] = True
        def place(cells, b, t):
            """cells: (m, 3) kind / column / row -> (m, 2) permutation position / row of the copy in tile (b, t)"""
            kind, col, row = cells[:, 0], cells[:, 1], cells[:, 2]
            adv = kind == 0
            colb = np.where(adv, lut[b][np.where(adv, col, 0)], col)
            p_ = np.where(adv, perm_adv[np.where(adv, colb, 0)], np.where(kind == 1, perm_fix[np.where(kind == 1, col, 0)], perm_inst[np.where(kind == 2, col, 0)]))
            assert (p_ >= 0).all(), "a copied cell lies in a column without equality enabled"
            return np.stack([p_, np.where(adv, row + t * U, row)], 1)
        chunks = [np.concatenate([place(first_tile[:, 0:3], 0, 0), place(first_tile[:, 3:6], 0, 0)], 1)]
        touches_blk = per_blk[np.where(unit[:, 0] == 0, unit[:, 1], 0)] & (unit[:, 0] == 0) | per_blk[np.where(unit[:, 3] == 0, unit[:, 4], 0)] & (unit[:, 3] == 0)
        for b in range(B):
            sub = unit if b == 0 else unit[touches_blk]                        # copies among shared columns only: once per tile, not once per block
            for t in range(T):
                if b == 0 and t == 0:
                    continue
                chunks.append(np.concatenate([place(sub[:, 0:3], b, t), place(sub[:, 3:6], b, t)], 1))
        copies = _CopyArray(np.concatenate(chunks))
        # advice: unit columns as canonical limbs, tiled; second-phase columns per proof (they depend on the challenges)
        self._U, self._T, self._colmap = U, T, colmap
        def tiled_col(vals):
            if as_ints:
                return list(vals[:U]) * T + [0] * (n - T * U)
            limbs = ints_to_limbs(vals[:U])
            out = np.zeros((n, 4), np.uint64)
            out[:T * U] = np.tile(limbs, (T, 1))
            return out
        phase_of = {c.index: c.phase for c in cs0.advice}
        def columns_of(region, phase):
            cols = {}
            for ci, vals in region.advice.items():
                if phase_of[ci] != phase:
                    continue
                t_ = tiled_col(vals)
                for cb in colmap.get(ci, [ci]):
                    cols[cb] = t_
            for c in cs0.advice:
                if c.phase == phase and c.index not in cols:
                    cols[c.index] = [0] * n if as_ints else np.zeros((n, 4), np.uint64)
            return cols
        first = columns_of(reg, 0)
        cache = {}
        def advice(phase, challenges):
            key = (phase, tuple(challenges))
            if key not in cache:
                if phase == 0:
                    cols = first
                else:
                    r2 = Region(cs0, self.k)
                    self._einsum(r2, tuple(challenges[:2]), A_in, B_in)
                    cols = columns_of(r2, 1)
                idx = sorted(cols)
                cache[key] = cols if as_ints else dict(zip(idx, limbs_to_mont([cols[i] for i in idx], gpu)))
            return cache[key]
        info = dict(circuit="transformer-shaped SURROGATE of configs[4] (not the nanoGPT graph): attention scores + softmax (exp, recip tables) + "
                            "layer norm (rsqrt table) + MLP + embedding gather (dynamic lookup) + transpose (shuffle) + %d x %d Freivalds einsum, "
                            "one unit of %d rows tiled %d x %d times, k=%d" % (self.L, self.L, U, T, B, self.k),
                    unit_rows=U, tiles=T, blocks=B, cells_used=int(reg.linear) * T * B)
        self.outputs = [v.v for v in h]
        out = dict(cs=cs, fixed=fixed, copies=copies, advice=advice, instances=[self.outputs], info=info)
        if synthesis == "device":                                              # (a failing lane raises here, as the host layout's assertion does above)
            _attach_device_witness(out, _DeviceSurrogateWitness(self, gpu, inputs, U, T, colmap))
        return out


def _check_synthesis(synthesis, gpu, as_ints):
    """the `synthesis` argument of a `build`, refused by name where it is unknown or cannot be served"""
    if synthesis not in ("host", "device"):
        raise ValueError("synthesis is \"host\" or \"device\", not %r" % (synthesis,))
    if synthesis == "device" and (gpu is None or as_ints):
        raise ValueError("synthesis=\"device\" needs a gpu backend and returns device columns")


def _attach_device_witness(out, dev):
    """a `build` result served from the device: `advice` replays the plan, `device_columns` names the resident columns, `witness` holds what
    to free, and the instance vector is read where phase 0 wrote it.  A witness the device refuses frees everything and raises."""
    out.update(witness=dev, advice=dev.advice, device_columns=list(range(dev.plan.n_advice)))
    try:
        dev.advice(0, [])
        out["instances"] = [dev.read_outputs()]
    except Exception:
        dev.free()
        raise


def host_phase_columns(circuit, x, first=None):
    """the advice columns of a circuit with phases from its HOST layout, phase by phase: those of phase 0 come from `first` (the first-phase
    region the caller already has; None: laid when first asked for), those of a phase p > 0 from the layout laid again with the
    challenges squeezed so far.  -> columns(phase, challenges) -> {column index: list of ints}"""
    cs0, n, regs = circuit.gc.cs, 1 << circuit.k, [first]
    def columns(phase, challenges):
        if phase == 0:
            reg = regs[0] = regs[0] if regs[0] is not None else circuit.synthesize(x, True)
        else:
            reg = circuit.synthesize(x, True, tuple(challenges[:len(cs0.challenges)]))
        return {c.index: reg.advice.get(c.index) or [0] * n for c in cs0.advice if c.phase == phase}
    return columns


class _DeviceWitness:
    """a circuit's witness made on the device: phase p replays phase p of the circuit's plan into one resident set of columns.
    phase_ms[p] = the device milliseconds of the last call."""

    def __init__(self, circuit, gpu, inputs, host_plan=None):
        from . import witness_plan as WP
        self.gpu, self.inputs, self.k = gpu, list(inputs), circuit.k
        self.plan = gpu.WitnessPlan((host_plan or WP.record_plan(circuit)).to_bytes())
        self.columns = self.plan.alloc_columns()
        self.outputs, self.phase_ms = None, {}

    def _ran(self, phase, run_ms):
        """what follows the replay of a phase -> its phase_ms entry"""
        return run_ms

    def advice(self, phase, challenges):
        phase = int(phase)
        _, outs = self.plan.run(self.inputs, columns=self.columns, phase=phase, challenges=list(challenges))
        self.phase_ms[phase] = self._ran(phase, self.plan.last["device_ms"])
        if phase == self.plan.n_phases - 1:
            self.outputs = outs
        return {c: self.columns[c] for c in range(self.plan.n_advice) if self.plan.column_phase[c] == phase}

    def set_inputs(self, inputs):
        """the inputs of the runs that follow (phase 0 takes them)"""
        if len(inputs) != self.plan.n_inputs:
            raise ValueError("the plan takes %d inputs, got %d" % (self.plan.n_inputs, len(inputs)))
        self.inputs = [int(v) for v in inputs]

    def read_outputs(self):
        """the circuit's outputs as canonical ints, gathered where phase 0 wrote them: one launch and one copy
        (backend.WitnessPlan.outputs; `run` hands them back with the plan's last phase only)"""
        return self.plan.outputs(self.columns)

    def free(self):
        for c in self.columns:
            c.free()
        self.columns = []
        self.plan.free()


class _DeviceSurrogateWitness(_DeviceWitness):
    """the surrogate's witness made on the device: the replay of a phase fills rows [0, U) of the block-0 and shared columns; the columns
    of that phase are then tiled (backend.witness_tile) -- U rows repeated T times down each column and into the columns of the other
    blocks.  phase_ms[p] = (run, tile) device milliseconds of the last call."""

    def __init__(self, circuit, gpu, inputs, U, T, colmap):
        from . import witness_plan as WP
        host_plan = WP.record_plan(circuit)
        super().__init__(circuit, gpu, inputs, host_plan)
        self.U, self.T = U, T
        # the columns the plan writes are tiled onto themselves and, those of block 0, into their blocks; the run of a phase zero-fills every
        # column of that phase first, the columns of blocks > 0 and the ones no record writes (phase 0) among them
        written, phase_of = sorted(WP.written_columns(host_plan)), self.plan.column_phase
        assert all(len(colmap.get(c, [c])) == 1 or colmap[c][0] == c for c in written), "the plan writes block-0 and shared columns only"
        self.pairs = {p: [(cb, c) for c in written if phase_of[c] == p for cb in colmap.get(c, [c])] for p in range(self.plan.n_phases)}

    def _ran(self, phase, run_ms):
        self.gpu.witness_tile(self.columns, self.k, self.U, self.T, self.pairs[phase])
        return run_ms, self.gpu.last_kernel_ms("witness_tile")                    # (reading the tile's events waits for it: the columns are final)


class PhasedLayoutCircuit(LayoutCircuit):
    """what the circuits share that lay Freivalds einsums over their own configuration (`BaseRegion.einsum`) and so have second-phase
    advice: `layout(reg, inputs, param, challenges=None) -> outputs` states the op sequence (`synthesize` runs it for one phase or for
    both), `build` gives keygen's and create_proof's inputs with a per-phase advice callable, on the host or from the witness plan.
    Subclasses give `layout`, `n_inputs`, `default_inputs()`, `plan_identity()` and `config()`."""
    lays_einsums = True

    def build(self, gpu=None, synthesis="host", as_ints=False, inputs=None):
        """-> dict(cs, fixed, copies, advice (callable(phase, challenges) -> {column: Montgomery array}), instances): the inputs of keygen
        and create_proof, as TransformerSurrogateCircuit.build gives them, without tiling.  as_ints: the advice callback returns lists of
        canonical ints (the MockProver's input).  inputs: X row-major (default: the seeded matrix).  synthesis: "host" -- the layout in
        Python, once per phase -- or "device" (needs gpu = ezkl_amd.backend): both phases replayed on the device from the circuit's
        witness plan; `advice` then returns {column: DeviceBuffer} of one resident set of columns, `device_columns` names them,
        `witness` holds what to free, and the instance vector is read from the plan's output cells."""
        _check_synthesis(synthesis, gpu, as_ints)
        inputs = self.default_inputs() if inputs is None else [int(v) for v in inputs]
        cs, fixed, copies, reg = self.keygen_inputs(inputs, with_witness=True)
        instances = [list(self.outputs)]
        columns, cache = host_phase_columns(self, inputs, reg), {}
        def advice(phase, challenges):
            key = (int(phase), tuple(challenges))
            if key not in cache:
                cols = columns(int(phase), challenges)
                cache[key] = cols if as_ints else dict(zip(cols, cols_to_mont(list(cols.values()), gpu)))
            return cache[key]
        out = dict(cs=cs, fixed=fixed, copies=copies, advice=advice, instances=instances)
        if synthesis == "device":
            _attach_device_witness(out, _DeviceWitness(self, gpu, inputs))
        return out


class AttentionHeadCircuit(PhasedLayoutCircuit):
    """One attention head over `n` tokens, every matmul a Freivalds einsum over the circuit's own configuration (layouts.rs:826 `einsum`,
    BaseRegion.einsum) -- the path the matmuls of a transformer graph take to the prover.  X (n x e) is the private model input, Wq, Wk,
    Wv (e x d) are parameters: Q, K, V = einsum("ie,ed->id"); S = einsum("id,jd->ij", Q, K), `div` by `score_div`, `softmax_axes` over the
    rows (the pieces of NormCircuit: max by sort, the exp table, sum, the claimed reciprocal, MULT -- outputs at input_scale *
    output_scale); O = einsum("ij,jd->id", P, V), `div` by input_scale * output_scale, range-checked and tied to the instance column.
    From the second einsum on the operands are cells the circuit computed.  The op sequence is stated once (`layout`).  The defaults keep
    the scores inside the exp table for entries of X in [-4, 4] and of the weights in [-2, 2] (`default_inputs`, the seeded weights);
    another input that leaves it is refused by the layout's own assertion."""

    def __init__(self, logrows, n, e, d, capacity, num_inner_cols=1, input_scale=8, output_scale=64, eps=1.0 / 128, score_div=None,
                 decomp_base=128, decomp_legs=2, lookup_range=(-255, 0), seed=1, Wq=None, Wk=None, Wv=None):
        """Wq, Wk, Wv: e x d integer matrices in place of the seeded ones (None: keep the seeded one)"""
        from . import einsum_plan as EP
        self.k, self.w, self.n, self.e, self.d, self.capacity = logrows, num_inner_cols, int(n), int(e), int(d), capacity
        self.n_inputs = self.n * self.e
        self.input_scale, self.output_scale, self.eps = int(input_scale), int(output_scale), float(eps)
        self.score_div = int(score_div) if score_div is not None else max(1, math.ceil(self.e * math.sqrt(self.d)))
        self.out_div = self.input_scale * self.output_scale
        self.base, self.legs, self.lookup_range, self.seed = decomp_base, decomp_legs, tuple(lookup_range), seed
        assert abs(zero_recip(self.output_scale, self.eps)) < decomp_base ** decomp_legs
        scale = self.input_scale
        self.exp = lambda x: int(math.floor(scale * math.exp(x / scale) + 0.5))         # LookupOp::Exp { scale, base: e } (ops.rs `exp`)
        self.equations = [("ie,ed->id", dict(i=self.n, e=self.e, d=self.d))] * 3 + [("id,jd->ij", dict(i=self.n, j=self.n, d=self.d)),
                                                                                   ("ij,jd->id", dict(i=self.n, j=self.n, d=self.d))]
        analyses = [EP.einsum_analysis(eq, dims) for eq, dims in self.equations]
        self.settings = EC.GraphSettings(logrows, num_inner_cols, capacity, total_const_size=16,
                                         required_range_checks=[(-1, 1), (0, decomp_base - 1), (0, 1)], required_lookups=[("exp", self.exp)],
                                         lookup_range=self.lookup_range, model_instance_shapes=[[self.n, self.d]],
                                         total_shuffle_col_size=self.n * self.n, num_shuffles=1,
                                         einsum_reduction_length=sum(a.reduction_length for a in analyses), einsum_max_output_axes=2)
        self.gc = EC.GraphConfig(self.settings)
        self.eins = [EinsumCircuit.over(self.gc, eq, dims) for eq, dims in self.equations]
        rng = np.random.default_rng(seed)
        self.Wq, self.Wk, self.Wv = (rng.integers(-2, 3, (self.e, self.d)) for _ in range(3))
        self.x = rng.integers(-4, 5, (self.n, self.e))
        _given_parameters(self, Wq=Wq, Wk=Wk, Wv=Wv)

    def default_inputs(self):
        return [int(v) for v in self.x.reshape(-1)]

    def layout(self, reg, inputs, param, challenges=None):
        """inputs: X row-major as `n_inputs` Vals; param(v) -> the Val of a circuit parameter (asked for in the order Wq, Wk, Wv, row-major);
        challenges: None lays the first phase (as the witness-plan recorder does, on symbols), else the two challenges: everything"""
        reg.decomp = (self.base, self.legs)
        n, d = self.n, self.d
        x = reg.assign(reg.inputs[0], inputs)                                        # placed once: the three projections read the same cells
        reg.increment(len(x))
        Wq, Wk, Wv = ([param(int(v)) for v in W.reshape(-1)] for W in (self.Wq, self.Wk, self.Wv))
        Q, K, V = (reg.einsum(ein, x, W, challenges) for ein, W in zip(self.eins[:3], (Wq, Wk, Wv)))
        S = reg.div(reg.einsum(self.eins[3], Q, K, challenges), self.score_div)
        P_ = reg.softmax_axes([S[i * n:(i + 1) * n] for i in range(n)], self.input_scale, self.output_scale, self.eps)
        O = reg.div(reg.einsum(self.eins[4], [v for row in P_ for v in row], V, challenges), self.out_div)
        return reg.output_equals_instance(O, self.gc.instance, 0, self.base, self.legs)

    def plan_identity(self):
        shape = [self.k, self.w, self.n, self.e, self.d, self.input_scale, self.output_scale, self.score_div, self.base, self.legs,
                 self.lookup_range[0], self.lookup_range[1], self.gc.advices[0].num_blocks()]
        return b"".join(np.asarray(a, np.int64).tobytes() for a in (shape, self.Wq, self.Wk, self.Wv)) + np.float64(self.eps).tobytes()

    def config(self):
        return dict(logrows=self.k, n=self.n, e=self.e, d=self.d, capacity=self.capacity, num_inner_cols=self.w, input_scale=self.input_scale,
                    output_scale=self.output_scale, eps=self.eps, score_div=self.score_div, decomp_base=self.base, decomp_legs=self.legs,
                    lookup_range=self.lookup_range, seed=self.seed, Wq=self.Wq, Wk=self.Wk, Wv=self.Wv)


class BatchMlpCircuit(PhasedLayoutCircuit):
    """MlpCircuit's op sequence on a BATCH: an m x k input matrix, m >= 2 rows through the same `layers` x (Gemm + bias + ReLU) in one
    proof -- ezkl's batch_size, and examples/onnx/large_mlp as the reference states it (9 x Linear(100, 100) + ReLU on a 10 x 100 batch).
    With m > 1 the Gemm "mk,nk->mn" has two non-common indices and the reference's analysis (einsum/analysis.rs:170-198) sends it to
    Freivalds' argument: every layer's product is an einsum over the circuit's own configuration (`BaseRegion.einsum`), second-phase
    advice and two challenges.  Private input and parameters, public output; the m * k inputs, row-major, and the m * n outputs are
    range-checked by decomposition.  The bias [1, n] is added to every row: layouts.rs `pairwise` (:2917) broadcasts both operands to
    [m, n] with `expand` (:3038, which repeats the VALUES -- a private parameter has no cell to share) and assigns all m * n entries of
    each, so the bias takes m * n cells of the second input column beside the m * n quotients, one ADD row per element, and the m
    copies of a bias entry are tied to nothing, as the entries of a private weight matrix are.
    A Gemm the analysis lays out with base ops -- m = 1, a layer with n = 1, or k = 1, where the sanitised equation has no common
    index -- is refused by name (ValueError): batch 1 is MlpCircuit's.  So is num_inner_cols != 1, the einsum layout's own rule: the RLC
    gate of a wider block folds num_inner_cols entries a row, which the witness plan's RLC record does not state."""

    def __init__(self, logrows, num_inner_cols, batch, weights, biases, decomp_base, decomp_legs, capacity=None, relu_last=True, relu_first=False,
                 rebase=None):
        """weights: per layer n x k integers; biases: per layer n; rebase: one divisor in [1, 2^32) per layer (MlpCircuit's), or None;
        capacity: the cells of a model column set (GraphSettings.total_assignments; None: counted)"""
        from . import einsum_plan as EP
        self.k, self.w, self.m = logrows, num_inner_cols, int(batch)
        self.weights = [[[int(v) for v in row] for row in W] for W in weights]
        self.biases = [[int(v) for v in b] for b in biases]
        self.base, self.legs, self.relu_last, self.relu_first = decomp_base, decomp_legs, bool(relu_last), bool(relu_first)
        self.rebase = [1] * len(self.weights) if rebase is None else [int(d) for d in rebase]
        if len(self.rebase) != len(self.weights) or any(not 1 <= d < 1 << 32 for d in self.rebase):
            raise ValueError("BatchMlpCircuit: rebase takes one divisor in [1, 2^32) per layer")
        if not self.weights:
            raise ValueError("BatchMlpCircuit: no layer (a Gemm-free graph is MlpCircuit's)")
        width = len(self.weights[0][0]) if self.weights[0] else 0
        self.equations = []
        for i, (W, b) in enumerate(zip(self.weights, self.biases)):
            if not W or any(len(row) != width for row in W) or len(b) != len(W) or width == 0:
                raise ValueError("BatchMlpCircuit: layer %d takes an n x %d weight matrix and n biases" % (i, width))
            dims = dict(m=self.m, k=width, n=len(W))
            if self.m < 1 or EP.einsum_analysis("mk,nk->mn", dims).strategy != EP.FREIVALDS:
                raise ValueError("BatchMlpCircuit: the Gemm of layer %d (m = %d, k = %d, n = %d) is %s%s"
                                 % (i, self.m, width, len(W), EINSUM_BASE_OPS_ERROR, " (batch 1 is MlpCircuit's)" if self.m == 1 else ""))
            self.equations.append(("mk,nk->mn", dims))
            width = len(W)
        if len(self.biases) != len(self.weights):
            raise ValueError("BatchMlpCircuit: one bias vector per weight matrix")
        if num_inner_cols != 1:
            raise ValueError("BatchMlpCircuit: num_inner_cols = %d: %s" % (num_inner_cols, EINSUM_WIDTH_ERROR))
        self.n_in, self.n_out = len(self.weights[0][0]), len(self.weights[-1])
        self.n_inputs = self.m * self.n_in
        self.capacity = int(capacity) if capacity is not None else self._count_cells()
        analyses = [EP.einsum_analysis(eq, dims) for eq, dims in self.equations]
        self.settings = EC.GraphSettings(logrows, num_inner_cols, self.capacity, total_const_size=16,
                                         required_range_checks=[(-1, 1), (0, decomp_base - 1)], model_instance_shapes=[[self.m, self.n_out]],
                                         einsum_reduction_length=sum(a.reduction_length for a in analyses), einsum_max_output_axes=2)
        self.gc = EC.GraphConfig(self.settings)
        self.eins = [EinsumCircuit.over(self.gc, eq, dims) for eq, dims in self.equations]

    def _count_cells(self):
        """an upper bound of the cells the layout places in a model column set (MlpCircuit._count_cells's terms, per batch element)"""
        dec = lambda c: _decomposition_cells(c, self.w, self.legs)
        c = dec(self.n_inputs)
        if self.relu_first:
            c += dec(self.n_inputs) + 6 * self.n_inputs
        for i, W in enumerate(self.weights):
            mn = self.m * len(W)
            if self.rebase[i] != 1:
                c += 3 * (dec(mn) + self.w) + 16 * mn
            c += mn
            if i + 1 < len(self.weights) or self.relu_last:
                c += dec(mn) + 6 * mn
        return c + 2 * dec(self.m * self.n_out) + self.m * self.n_out + 64

    def default_inputs(self):
        return [(7 * i + 3) % 11 - 5 for i in range(self.n_inputs)]

    def layout(self, reg, inputs, param, challenges=None):
        """inputs: the m x k matrix row-major as `n_inputs` Vals; param(v) -> the Val of a circuit parameter (asked for per layer: the
        weight matrix row-major, then the biases); challenges: None lays the first phase (as the witness-plan recorder does, on
        symbols), else the two challenges: everything"""
        reg.decomp = (self.base, self.legs)
        _, vals = reg.decompose(inputs, self.base, self.legs)                   # input range check
        if self.relu_first:
            vals = reg.relu(vals, self.base, self.legs)
        for i, (W, b, ein) in enumerate(zip(self.weights, self.biases, self.eins)):
            outs = reg.einsum(ein, vals, [param(wv) for row in W for wv in row], challenges)      # the Gemm: a Freivalds einsum
            outs = reg.div(outs, self.rebase[i])                                   # RebaseScale around the Einsum node
            bias = [param(bv) for bv in b]
            vals = reg.pairwise(outs, bias * self.m, EC.ADD)                       # [1, n] broadcast over the m rows: m * n cells
            if i + 1 < len(self.weights) or self.relu_last:
                vals = reg.relu(vals, self.base, self.legs)
        return reg.output_equals_instance(vals, self.gc.instance, 0, self.base, self.legs)

    def plan_identity(self):
        shape = [self.k, self.w, self.m, self.base, self.legs, int(self.relu_last), int(self.relu_first), len(self.weights),
                 self.gc.advices[0].num_blocks()]
        per_layer = [a for W, b in zip(self.weights, self.biases) for a in ([len(W), len(W[0])], W, b)]
        return b"".join(np.asarray(a, np.int64).tobytes() for a in [shape] + per_layer + [self.rebase])

    def config(self):
        return dict(logrows=self.k, num_inner_cols=self.w, batch=self.m, weights=self.weights, biases=self.biases, decomp_base=self.base,
                    decomp_legs=self.legs, relu_last=self.relu_last, relu_first=self.relu_first, capacity=self.capacity, rebase=self.rebase)


def limbs_to_mont(cols, gpu=None):
    """(n, 4) canonical limb arrays -> Montgomery arrays (on the device when a backend is given: one product by R^2 per element)"""
    if gpu is None:
        M = (1 << 256) % R
        out = []
        for a in cols:
            ints = [int.from_bytes(a[i].tobytes(), "little") for i in range(a.shape[0])]
            out.append(np.frombuffer(b"".join((v * M % R).to_bytes(32, "little") for v in ints), np.uint64).reshape(-1, 4).copy())
        return out
    r2 = P.to_mont((1 << 256) % R)
    out = []
    for a in cols:
        buf = gpu.DeviceBuffer.from_numpy(np.ascontiguousarray(a))
        gpu.vec_scale(buf.ptr, r2, buf.ptr, a.shape[0])
        pa = gpu.PinnedArray((a.shape[0], 4))             # page-locked: what a prover's synthesis should fill (uploads at PCIe speed)
        pa.array[:] = buf.to_numpy(shape=(a.shape[0], 4))
        _PINNED.append(pa)
        out.append(pa.array)
        buf.free()
    return out
