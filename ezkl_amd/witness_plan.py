"""Witness plans: the layout of an MlpCircuit, a ConvMnistCircuit, an EinsumMatmulCircuit, an EinsumCircuit, a SumProdLayoutCircuit, a
SortTopkCircuit, a NormCircuit, a PoolClassifierCircuit, a ScatterGatherCircuit, an AttentionHeadCircuit or the TransformerSurrogateCircuit's
unit recorded ONCE, replayed for every proof.

Which advice cell holds which value depends only on the circuit (BaseRegion places cells from the linear coordinate, the duplicated rows
of `dot` from the block geometry; constants and the circuit's parameters are the same for every input), so `record_plan` runs one
witness-free layout pass over a BaseRegion subclass whose VALUES are symbols: the op sequence that runs is the circuit's own, stated once
(`layout`, which its `synthesize` runs on values; the einsum's `sequence`) -- no circuit's ops or parameters are spelt out in this module
--, the placement code is BaseRegion's own (cell_of, flush, _dup_inputs, the duplicate row at the top of a new column, every layouts.rs
op as BaseRegion lays it out), and every `put` records how the cell it wrote is produced from earlier cells, a model input, a circuit
parameter or a constant.  The cell writes are grouped into RECORDS -- one kernel launch each on the device (csrc/witness.hip) -- by data
dependence.  An MlpCircuit -- with or without the rebase division of its layers (`BaseRegion.div`: one DIVC record per layer for the claimed
quotients, everything else of the op is records of the kinds the family already had) -- is recorded on a RecordingRegion: a write joins the latest record of its kind when everything it reads was
written by an earlier record, so the 650 dot products of a layer are one record, not 650.  (Every other circuit with a `layout` is
recorded on a LookupRecordingRegion and grouped by dependence LEVEL: a write joins the EARLIEST record of its kind
that comes after every record it reads from.  A cell is written once and read only by writes later in program order, so no element
of an existing record can depend on the cell that joins it.  The conv loop alternates dot and add and copies its patches from early
cells: under the latest-fit rule every patch copy lands behind the previous dot and forces a new dot record, 1751 records for the conv +
ReLU part at k = 17; by levels it is 25.  The MLP path keeps the latest-fit rule: its blobs stay what they were.)
The LookupRecordingRegion also records the rest of the layout engine's ops: `sum` / `prod` (one SUMACC / PRODACC scan each), `dynamic_lookup`
and `shuffle` (both sides of the argument are placed through `put`: parameter, constant, input or copy records; a pick whose row is chosen
by a VALUE -- `BaseRegion.row_at`, the embedding gather -- is the index itself in the key coordinate and a GATHER element over the cells of
the dynamic table in every other one; `shuffle` in a data-dependent order is refused by name), `ezkl_layout.clamped` (a CLAMP record) and
`sort_ascending` / `topk` (`BaseRegion._sorted`, the one data-dependent step, is a SORT segment for the sorted values and an ARGSORT segment
for the claimed indices; everything around it is records of the other kinds), and `recip` / `sqrt` with what is built on them (`rsqrt`,
`percent`, `softmax`, `mean_of_squares`): the claimed reciprocal is a RECIP element, the claimed root an ISQRT element
(`ezkl_layout.recip_claim` / `sqrt_claim`, the two data-dependent steps), the masks, products, distances and comparisons of
`optimum_convex_function` around them are records of the other kinds, `max` is a sort and `exp` a static lookup.  `argmax` / `argmin`
claim their index BEFORE the sort that checks it (`BaseRegion._arg_extremum`, the one data-dependent step): the claim is one segment of an
ARGEXT record, the `select` around it a gather, the rest a sort; `max_pool` is a `max` per window and `sumpool` a `dot` per window plus `div`.
The indexed family -- `gather`, `gather_elements`, `scatter_elements`, `get_missing_set_elements`, `one_hot` -- has three claims that depend on the
data: the scattered tensor, claimed before the gathers that check it (`BaseRegion._scattered`: one SCATTER record), the complement of the
written positions (`_missing`: one COMPLEMENT record) and the one-hot vector (`_one_hot`: ONEHOT elements); the many-pick `select_elements`
is GATHER elements over one table, the claimed indices of the missing set's permutation argument are copies, the rest records of the other kinds.
The MLP recorder keeps refusing them by name.  The TransformerSurrogateCircuit lays its einsum over its own configuration
(`BaseRegion.einsum`): it is recorded on a PhasedLookupRecordingRegion -- the lookup region with the einsum region's `put_cell`, matmul
record, running values and phase bookkeeping -- into a TWO-phase plan of the unit's rows; the tiling is the device's
(ezkl_hip_witness_tile_dev).
An EinsumCircuit -- any two-operand equation of the Freivalds chip -- standing alone or laid over an AttentionHeadCircuit's configuration
is recorded from its own `sequence` too (EinsumRecordingRegion.lay_einsum): its operands may be cells the circuit computed, and the product
the prover claims is ONE DOT record of one step over those cells, emitted after them although the layout writes it before them.

The plan is a flat little-endian blob (`WitnessPlan.to_bytes`):

    header   20 x u32: magic "EZWP", version, k, n_advice, n_records, n_inputs, n_params, n_consts, n_outputs, n_cells, n_words, n_ops,
             n_tables, n_table_values, n_challenges, n_phases (0 reads as 1: a one-phase plan writes 0, the reserved word it was), 4 reserved
             (zero); then the 32-byte parameter hash
    params   n_params  x int64        in the order the circuit's `layout` asks for them (fixed at record time)
    consts   n_consts  x 32 bytes     canonical field elements
    records  n_records x 8 u32        kind, count, p0, p1, dst, a, b, phase   (dst / a / b: word offsets into the pool)
    outputs  n_outputs x u32          the cells that hold the circuit's outputs
    pool     n_words   x u32          cell indices (column * 2^k + row), table indices, per-element arguments
    tables   n_tables  x 4 u32        lo (int32), n (entries), col_size, offset into the values      } both sections are empty in a plan
    values   n_table_values x int64   f(lo + i) of a static lookup table, as a signed integer        } without lookups: the MLP blobs

THE RECORD KINDS, by number; `KINDS` below is the same list as a table (name, run-time failure, span shape) and csrc/witness_plan.hpp holds
its twin.  Kinds 16, 23, 26 and 28 are unassigned and refused as unknown, as is everything from KINDS_TOP = 32 on.  Unless an entry says
otherwise a record is element-wise: `count` destination cells pool[dst + i], produced from pool[a + i] (and pool[b + i]); b unused is zero;
s is the signed value of the source cell.  A run-time failure is a lane's: reported as "<words> (<kind> record r, element e)", here by
`run_plan_host` and on the device through the status words; the lane writes nothing.

     0 COPY    a = source cell
     1 CONST   a = constant index
     2 INPUT   a = input index
     3 PARAM   a = parameter index
   4-6 ADD, SUB, MUL   a, b = source cells
     7 HINT    a = source cell, b = 0xffffffff: the sign of s; else the digit (|s| // p0^b) % p0; p0 = base >= 2, p1 = legs >= 1, p0^p1 < 2^62 and
               every digit below p1 ("bad decomposition").  |s| >= p0^p1 fails: "value exceeds the decomposition range"
     8 RCIDX   a = source cell: |s - p0| // p1 (p0 = the range's lower end as int32, p1 = the table column size >= 1).  |s| >= 2^62 -- more than a
               lane holds in 64 bits, never a sign or a digit -- fails with the decomposition-range words
     9 INVZ    a = source cell: 1 / x, or 0 for x = 0
    10 DOT     count dot products of p1 steps of p0 products each, step-major: step t of dot d writes the running sum to pool[dst + t * count + d]
               (0xffffffff: no such step) after adding the products of pool[a + (t * p0 + j) * count + d] and pool[b + ...] (0xffffffff in both:
               none -- the duplicated running sum at the top of a new column is a step without products)
               An einsum's claimed product is such a record with p1 = 1 and p0 = the contracted index tuples, 2 * p0 * count <= 2^28 pool words;
               from p0 = DOT_WIDE_MIN on the device runs a one-step record on a kernel of its own (dot_wide_lanes lanes to a dot): same cells
    11 TABLE   a = source cell, p0 = table index: values[offset + (s - lo)] as a field element (a negative value as integer_rep_to_felt maps it)
    12 TBLIDX  a = source cell, p0 = table index: (s - lo) // col_size, the table column that holds s.  Both: s < lo, s > lo + n - 1 or
               |s| >= 2^62 fails: "lookup input outside the table range"
    13 MATMUL  count = m * n outputs, p0 = kd, p1 = n: pool[dst + i * n + j] = sum_t in[pool[a + i * kd + t]] * in[pool[b + t * n + j]] over the
               INTEGERS, then integer_rep_to_felt -- the product the prover witnesses (EinsumMatmulCircuit.matmul); a: m * kd, b: kd * n input
               indices; phase 0.  An operand with |v| >= 2^31 (the sum would not fit 128 bits) fails: "einsum operand outside the exact-product
               range", element = the operand's place in a, or m * kd + its place in b; the count is of operand reads
    14 RLC     count scans of p1 steps with challenge p0 (< n_challenges), step-major and dense: out[0] = c * v[0], out[t] = out[t - 1] * c + c * v[t]
               with v[t] = the cell pool[a + t * count + d], out[t] -> pool[dst + t * count + d]   (RLCConfig::assign_rlc at block width 1)
    15 DIVC    a = source cell, p0 = d >= 1 ("zero divisor"), p1 = 0: sgn(s) * ((|s| + d // 2) // d) -- s / d rounded half away from zero, the
               claimed quotient of `div` (ezkl_layout.round_div).  |s| >= 2^52 fails: "rebase dividend outside the exact-division range"
 17, 18 SUMACC, PRODACC   count scans of p1 steps with p0 operands each, step-major as DOT is: step t of scan d folds the cells
               pool[a + (t * p0 + j) * count + d], j < p0 (0xffffffff: no operand -- the duplicated row at the top of a new column), into the running
               value (0 at the start of a sum, 1 of a product) and writes it to pool[dst + t * count + d] (0xffffffff: the scan has no such step: a
               ragged record).  p0 or p1 zero, or an array past the pool: "bad scan shape"   (BaseRegion._accumulate, layouts.rs:2472-2621)
    19 GATHER  a = the cell holding the index, p0 = the pool offset of the table's cell list, p1 = its length n >= 1 ("empty gather table", "gather
               table runs past the pool"); every cell of the list is one a lane can read.  The value of cell pool[p0 + s].  s < 0, s >= n or
               |s| >= 2^62 fails: "gather index outside the table"; the lane tests s before it reads pool[p0 + s]
    20 CLAMP   a = source cell, p0 = lo, p1 = hi (int32, lo <= hi, else "bad clamp bounds"): min(max(s, lo), hi); a value beyond 62 bits clamps by
               its sign; never fails
 21, 22 SORT, ARGSORT   count destination cells pool[dst + e] in segments of p0 = n elements (n >= 1, count % n == 0, count <= 2^28), p1 = mode
               (0: position ascending among equal values, 1: descending; anything else of these: "bad sort shape"), a = the source cells,
               segment-major and dense.  The order of a segment is by (signed value, position) -- a total order.  SORT: destination g * n + i gets
               the i-th smallest signed value of the cells pool[a + g * n .. + n) as integer_rep_to_felt maps it; ARGSORT: the position, in
               [0, n), of that element in its segment (BaseRegion.sort_ascending, layouts.rs:1158-1275 with the claimed indices of `shuffles`,
               :1624-1760).  A source with |s| >= 2^62 fails: "sort key beyond 62 bits", element = its place in a; on the device its segment
               writes none of its cells.  SORT_TILE is the number of keys one workgroup sorts in LDS
    24 RECIP   a = source cell, b = the index in the constants section of `zero_inverse` (ONE word for the record, not a pool offset: "zero-inverse
               index past the constants"), p0 / p1 = the low / high word of S = input_scale * output_scale, 1 <= S < 2^62 ("reciprocal scale
               outside [1, 2^62)").  s = 0 -> that constant; s > 0 -> ceil((2S - s) / (2s)); s < 0 -> -floor((2S + |s|) / (2|s|)): the smallest
               integer minimiser of |y * s - S| (ezkl_layout.recip_claim).  |s| >= 2^62 fails: "reciprocal operand beyond 62 bits"
    25 ISQRT   a = source cell, p0 = the input scale >= 1 ("zero square-root scale"), p1 = 0 ("a square-root record with a second parameter").
               With T = s * p0: T <= 0 -> 0, else r = isqrt(T), r + (T - r * r > r): the integer nearest to sqrt(T) (ezkl_layout.sqrt_claim).
               |s| >= 2^62 or T >= 2^62 fails: "square-root operand outside the exact range"
    27 ARGEXT  count segments of p0 = n >= 1 source cells and as many destination cells pool[dst + g], p1 = mode (0: argmax, 1: argmin), a = the
               count * n <= 2^28 source cells, segment-major and dense (else "bad arg-extremum shape").  Destination g gets the SMALLEST position
               j in [0, n) whose signed value is the greatest (mode 0) or the least (mode 1) of the cells pool[a + g * n .. + n): the claimed
               index of `argmax` / `argmin` (BaseRegion._arg_extremum, layouts.rs:5225-5293), the one claim the gates accept.  A source with
               |s| >= 2^62 fails: "arg-extremum key beyond 62 bits", element = its place in a; on the device its segment's cell is not written.
               ARGEXT_CHUNK is the number of sources one workgroup reduces
    29 SCATTER ONE tensor: count = n destination cells pool[dst + i], a = the n base cells, p0 = m >= 1 elements, p1 = the multiplier of the
               scattered dimension >= 1, b = the pool offset of 1 + 3m words: the extent of that dimension, m index cells, m source cells, m
               constant offsets (plain u32, not cells).  With s_j the signed value of index cell j its target is t_j = s_j * p1 + off_j;
               destination i gets the value of source cell j for the GREATEST j with t_j == i, else the value of base cell i: the claimed output
               of `scatter_elements` (BaseRegion._scattered, layouts.rs:2313-2379, `tensor::ops::scatter`: the later element wins).  p0, p1 or the
               extent zero, count > 2^28, an array past the pool or an offset with off_j + (extent - 1) * p1 >= count: "bad scatter shape" -- so
               every target of an index inside [0, extent) is a destination.  s_j < 0, s_j >= extent or |s_j| >= 2^62 fails: "scatter index
               outside the tensor", element = j, every such j counted; the record then writes none of its cells.  SCATTER_TILE is the number of
               destinations one workgroup resolves in LDS
    30 COMPLEMENT   p0 = n: the set {0 .. n - 1}, p1 = m <= n source cells at a, count = n - m destination cells (zero is legal: the record writes
               nothing).  Destination i gets the i-th smallest v in [0, n) that is the signed value of no source cell: the claimed output of
               `get_missing_set_elements` over the positions (BaseRegion._missing, layouts.rs:2213-2286).  A source outside [0, n) or beyond 62
               bits removes nothing; never fails.  p1 > p0, count != p0 - p1, p0 > 2^28 or an array past the pool: "bad complement shape"
    31 ONEHOT  a = the index cell of element e, b = the pool offset of the per-element positions (plain u32), p0 = num_classes >= 1 ("zero
               one-hot classes"), p1 = 0: 1 if s equals the position, else 0 (BaseRegion._one_hot, layouts.rs:1398-1442).  s < 0, s >= p0 or
               |s| >= 2^62 fails: "one-hot index outside the classes"

PHASES.  A circuit with second-phase advice (the Freivalds einsum) has columns that depend on challenges squeezed after the first-phase
commitments: its plan has n_phases = 2, and every record carries the phase whose run replays it.  Phases are non-decreasing along the
record list; a column belongs to the phase of the records that write it (never to two; a column no record writes: phase 0); INPUT and
MATMUL records belong to phase 0, with which the inputs are uploaded.  A later phase reads the cells of an earlier one where they are.

COUPLING WITH ezkl_layout.py.  The recorder reuses BaseRegion's value expressions too, by operator overloading on the symbols below, and
recognises them AS THEY ARE SPELT there.  Whoever rewrites one of these lines of BaseRegion must extend the symbol classes with it (the
equality tests of tests/test_witness_plan_cpu.py fail loudly -- an assert or a PlanError during recording -- until then):
    decompose / range_check   `s = v if v < R // 2 else v - R`   (a comparison with exactly R // 2 answers True: the symbol IS the signed value)
    decompose                 `(s > 0) - (s < 0)`, `abs(s)`, `(mag // base ** e) % base`, `assert mag < base ** legs` (recorded as the run-time check)
    range_check               `abs(s - lo) // col_size`
    pairwise                  `x + y`, `x - y`, `x * y` on two assigned cells
    dot                       `acc = (acc + sum(x.v * y.v for ...)) % R` with acc and sum() starting from the integer 0
    sum (_accumulate)         `(acc + sum(chunk)) % R` with acc and sum() starting from the integer 0, chunk = the w cells of the row
    prod (_accumulate)        `acc = acc * v % R` over the w cells of the row, acc starting from the integer 1
    clamped (module level)    `s.clamped(lo, hi)` when the signed value is a symbol, `min(max(s, lo), hi)` otherwise
    recip_claim (module level) `s.recip_claim(S, zero_inverse)` when the signed value is a symbol; in `recip`: `recip_claim(signed(v.v), S, zero_inverse)`
    sqrt_claim (module level) `s.sqrt_claim(scale)` when the signed value is a symbol; in `sqrt`: `sqrt_claim(signed(v.v), int(input_scale))`
                              (`signed`: `v if v < R // 2 else v - R`, as above: the symbol IS the signed value)
    _sorted                   overridden: `assert abs(s) < 1 << 62` is the run-time check of SORT / ARGSORT
    row_at                    overridden: `assert 0 <= signed(index.v) < len(table_rows)` is the run-time check of GATHER
    _arg_extremum             overridden: `assert abs(x) < 1 << 62` is the run-time check of ARGEXT
    _scattered                overridden: `assert 0 <= s < dims[dim] and abs(s) < 1 << 62` is the run-time check of SCATTER; the offsets are
                              `sum(coord[t] * mult[t] for t != dim)` of BaseRegion._strides / _coords
    _missing                  overridden: the full set must be the constants 0 .. n - 1 (COMPLEMENT); it never fails
    _one_hot                  overridden: `assert 0 <= s < num_classes and abs(s) < 1 << 62` is the run-time check of ONEHOT
    _claimed_indices          overridden: over the constants 0 .. n - 1 the claimed index of an output element is its own value (a COPY)
    select_elements           every pick goes through `row_at`, as `select`'s one pick does: GATHER elements over one table
    equals_zero               `pow(v, -1, R) if v else 0`   (the truth value of a cell symbol is True: INVZ covers both branches)
    div (round_div)           `mag = abs(s)`, `assert mag < 1 << 52` (recorded as the run-time check), `((s > 0) - (s < 0)) * ((mag + d // 2) // d)`
    nonlinearity              `assert table.range[0] <= signed(v) <= table.range[1]` (recorded as the run-time check), `table.f(signed(v)) % R`,
                              `(signed(v) - table.range[0]) // table.col_size` -- LookupRecordingRegion only; `table` is its stand-in there;
                              `lookup_inputs_seen` (the running extrema of a witness file) is overridden to nothing: `lookup_stats_host` and
                              the device compute them from the replayed cells
    Val.__init__ and the ops  `... % R` on any symbol is the symbol

Every cell is written at most once and only reads cells of earlier records; `validate` checks that (the C library runs the same check
on upload).  `run_plan_host` interprets the blob with Python integers: the executable specification of the device kernels."""
import bisect
import collections
import hashlib
import struct

import numpy as np

from . import ezkl_layout as EL

R = EL.R
MAGIC, VERSION = 0x50575A45, 1                  # "EZWP"
NONE = 0xFFFFFFFF
COPY, CONST, INPUT, PARAM, ADD, SUB, MUL, HINT, RCIDX, INVZ, DOT, TABLE, TBLIDX, MATMUL, RLC, DIVC = range(16)
SUMACC, PRODACC, GATHER, CLAMP, SORT, ARGSORT = range(17, 23)
RECIP, ISQRT, ARGEXT = 24, 25, 27
SCATTER, COMPLEMENT, ONEHOT = 29, 30, 31
KINDS_TOP = 32                                     # the first kind past them all
SORT_TILE, MAX_SORT_COUNT = 2048, 1 << 28                       # csrc/witness_plan.hpp: the keys one workgroup sorts in LDS; the most cells of a sort record
ARGEXT_CHUNK = 4096                                             # csrc/witness_plan.hpp: the sources one workgroup of an arg-extremum reduces
SCATTER_TILE = 4096                                             # csrc/witness_plan.hpp: the destinations one workgroup of a scatter / a complement resolves in LDS
DOT_WIDE_MIN, DOT_WIDE_FILL = 16, 1 << 17                       # csrc/witness_plan.hpp: a DOT record of one step with this many products runs on the wide kernel; the lanes that fill the device
MAX_CLAIM_WORDS = 1 << 28                                       # the most pool words (2 * K * |O|) of an einsum's claim
CLAIM_ERROR = "an einsum claim of more than 2^28 pool words"


def dot_wide_lanes(count, p0):
    """csrc/witness_plan.hpp dot_wide_lanes: how many lanes of a wave share one dot of the wide kernel -- a power of two, at most 64 and at
    most p0; one when `count` dots alone fill the device, more when there are few long dots"""
    g = 1
    while g < 64 and 2 * g <= p0 and count * g < DOT_WIDE_FILL:
        g *= 2
    return g
_HEADER = struct.Struct("<20I32s")
RANGE_ERROR = "value exceeds the decomposition range"
LOOKUP_ERROR = "lookup input outside the table range"
OPERAND_ERROR = "einsum operand outside the exact-product range"
DIV_ERROR = EL.DIV_ERROR
GATHER_ERROR = "gather index outside the table"
SORT_ERROR = EL.SORT_ERROR
RECIP_ERROR, SQRT_ERROR = EL.RECIP_ERROR, EL.SQRT_ERROR
ARGEXT_ERROR = EL.ARGEXT_ERROR
SCATTER_ERROR, ONEHOT_ERROR = EL.SCATTER_ERROR, EL.ONEHOT_ERROR
MAX_PHASES, MAX_CHALLENGES = 3, 64

# The table of record kinds, the same as KINDS of csrc/witness_plan.hpp (tests/test_witness_plan_table.py): the name a message gives the kind,
# the words of its run-time failure (None: a lane of this kind never fails), what that failure counts, whether the record has count * p1
# destination words (a scan) or count, whether 0xffffffff in dst, a or b is "no entry", and what the words at a and at b are: cells a lane
# reads, indices below a limit the kind's case names (DIGITS: 0xffffffff too, the sign), plain words (none where the kind does not use the
# array), or no pool offset at all.
CELLS, INDICES, DIGITS, WORDS, NOT_POOL = "cells", "indices", "digits", "words", "not a pool offset"
Kind = collections.namedtuple("Kind", "name failure unit scan sparse a b", defaults=(None, "cells", False, False, CELLS, WORDS))
_ASSIGNED = {
    COPY: Kind("copy"), CONST: Kind("const", a=INDICES), INPUT: Kind("input", a=INDICES), PARAM: Kind("param", a=INDICES),
    ADD: Kind("add", b=CELLS), SUB: Kind("sub", b=CELLS), MUL: Kind("mult", b=CELLS),
    HINT: Kind("decompose", RANGE_ERROR, b=DIGITS), RCIDX: Kind("range_check", RANGE_ERROR), INVZ: Kind("equals_zero"),
    DOT: Kind("dot", scan=True, sparse=True, b=CELLS), TABLE: Kind("nonlinearity", LOOKUP_ERROR), TBLIDX: Kind("nonlinearity_index", LOOKUP_ERROR),
    MATMUL: Kind("matmul", OPERAND_ERROR, "operand reads", a=INDICES, b=INDICES), RLC: Kind("rlc", scan=True), DIVC: Kind("div", DIV_ERROR),
    SUMACC: Kind("sum", scan=True, sparse=True), PRODACC: Kind("prod", scan=True, sparse=True), GATHER: Kind("gather", GATHER_ERROR), CLAMP: Kind("clamp"),
    SORT: Kind("sort", SORT_ERROR), ARGSORT: Kind("argsort", SORT_ERROR), RECIP: Kind("recip", RECIP_ERROR, b=NOT_POOL), ISQRT: Kind("sqrt", SQRT_ERROR),
    ARGEXT: Kind("argext", ARGEXT_ERROR), SCATTER: Kind("scatter", SCATTER_ERROR), COMPLEMENT: Kind("complement"), ONEHOT: Kind("one_hot", ONEHOT_ERROR),
}
KINDS = [_ASSIGNED.get(kind, Kind("?", a=WORDS)) for kind in range(KINDS_TOP)]
UNASSIGNED_KINDS = tuple(kind for kind in range(KINDS_TOP) if kind not in _ASSIGNED)      # (16, 23, 26, 28): they name nothing and never will; refused as unknown
KIND_NAMES = [K.name for K in KINDS]               # "?" in the four holes


class PlanError(ValueError):
    pass


def kind_name(kind):
    """the name a message gives a record kind; "?" for a number that names nothing"""
    return KIND_NAMES[kind] if 0 <= kind < KINDS_TOP else "?"


def dst_words(kind, count, p1):
    """how many destination words a record has: every step of every scan, else one per element"""
    return count * p1 if KINDS[kind].scan else count


# ---- symbolic values: what a Val's .v holds during the recording pass -------------------------------------------------------------------
class _Sym:
    """a value the layout does arithmetic on; only the forms BaseRegion's ops use exist, anything else is refused by name"""
    __hash__ = object.__hash__

    def __mod__(self, m):                          # Val.__init__ and the ops reduce mod r
        assert m == R
        return self

    def _no(self, *a, **kw):
        raise PlanError("the witness plan recorder does not cover this use of a %s value" % type(self).__name__)
    __add__ = __radd__ = __sub__ = __rsub__ = __mul__ = __rmul__ = __floordiv__ = __lt__ = __gt__ = __le__ = __ge__ = __abs__ = __pow__ = _no
    __bool__ = __int__ = __index__ = _no


class _Cell(_Sym):
    """the value of an advice cell written earlier"""

    def __init__(self, idx): self.idx = idx
    def __add__(self, o): return _Bin(ADD, self, o)
    def __sub__(self, o): return _Bin(SUB, self, o) if isinstance(o, _Cell) else _Shift(self, o)
    def __mul__(self, o): return _Bin(MUL, self, o)
    def __lt__(self, o): return True if o == R // 2 else _Cmp(self, "<", o)     # `v if v < R // 2 else v - R`: the signed value is the symbol itself
    def __gt__(self, o): return _Cmp(self, ">", o)
    def __ge__(self, o):                           # `lo <= s <= hi`, the lookup's range assertion: recorded, checked by `put` and at run time
        self.lo = o
        return True
    def __le__(self, o):
        self.hi = o
        return True
    def __abs__(self): return _Mag(self)
    def __bool__(self): return True                                             # `pow(v, -1, R) if v else 0` is INVZ either way
    def __pow__(self, e, m=None):
        assert e == -1 and m == R
        return _Un(INVZ, self)
    def __radd__(self, o):                         # sum(chunk) starts from 0: the operands of one step of `sum`
        if not (isinstance(o, int) and o == 0):
            self._no()
        return _Operands([self.idx])
    def __rmul__(self, o):                         # `acc * v` with acc = 1: the first operand of the first step of `prod`
        if not (isinstance(o, int) and o == 1):
            self._no()
        return _Fold(PRODACC, None, [self.idx])
    def clamped(self, lo, hi): return _Clamp(self, lo, hi)      # ezkl_layout.clamped on the signed value
    def recip_claim(self, S, zero_inverse): return _Recip(self, S, zero_inverse)     # ezkl_layout.recip_claim on the signed value
    def sqrt_claim(self, scale): return _Isqrt(self, scale)                          # ezkl_layout.sqrt_claim on the signed value


class _Input(_Sym):
    def __init__(self, idx): self.idx = idx


class _Param(_Sym):
    def __init__(self, idx): self.idx = idx


class _Bin(_Sym):
    def __init__(self, kind, a, b):
        if not (isinstance(a, _Cell) and isinstance(b, _Cell)):
            self._no()
        self.kind, self.a, self.b = kind, a.idx, b.idx

    def __radd__(self, o):                         # sum(products) starts from 0
        assert self.kind == MUL and o == 0
        return _Products([(self.a, self.b)])


class _Products(_Sym):
    """the w products of one dot step"""

    def __init__(self, pairs): self.pairs = pairs
    def __add__(self, o):
        assert isinstance(o, _Bin) and o.kind == MUL
        return _Products(self.pairs + [(o.a, o.b)])
    def __radd__(self, o):                         # acc + products, acc = 0 on the first step
        assert o == 0
        return _Acc(None, self.pairs)


class _Acc(_Sym):
    """a running dot sum: the previous running sum (None on the first step) plus this step's products; `cell` once it has been put"""

    def __init__(self, prev, pairs): self.prev, self.pairs, self.cell = prev, pairs, None
    def __add__(self, o):
        assert isinstance(o, _Products)
        return _Acc(self, o.pairs)


class _Un(_Sym):
    def __init__(self, kind, a): self.kind, self.a = kind, a.idx


class _Operands(_Sym):
    """the w cells one step of `sum` adds"""

    def __init__(self, cells): self.cells = cells
    def __add__(self, o):
        if not isinstance(o, _Cell):
            self._no()
        return _Operands(self.cells + [o.idx])
    def __radd__(self, o):                         # acc + sum(chunk), acc = 0 on the first step
        if not (isinstance(o, int) and o == 0):
            self._no()
        return _Fold(SUMACC, None, self.cells)


class _Fold(_Sym):
    """a running sum or product (`_accumulate`): the previous running value (None on the first step) folded with this step's cells; `cell`
    once it has been put"""

    def __init__(self, kind, prev, cells): self.kind, self.prev, self.cells, self.cell = kind, prev, cells, None
    def __add__(self, o):
        if not (self.kind == SUMACC and isinstance(o, _Operands) and self.cell is not None):
            self._no()
        return _Fold(SUMACC, self, o.cells)
    def __mul__(self, o):                          # the next operand of this step, or -- once the running value is placed -- of the next
        if not (self.kind == PRODACC and isinstance(o, _Cell)):
            self._no()
        return _Fold(PRODACC, self, [o.idx]) if self.cell is not None else _Fold(PRODACC, self.prev, self.cells + [o.idx])


class _Clamp(_Sym):
    def __init__(self, a, lo, hi): self.a, self.lo, self.hi = a.idx, lo, hi


class _Recip(_Sym):
    """the claimed reciprocal of cell a at S = input_scale * output_scale; `zero_inverse` for a zero"""

    def __init__(self, a, S, zero_inverse): self.a, self.S, self.zero_inverse = a.idx, S, zero_inverse


class _Isqrt(_Sym):
    """the claimed square root of cell a times `scale`"""

    def __init__(self, a, scale): self.a, self.scale = a.idx, scale


class _Pick:
    """one data-dependent pick of a dynamic lookup (`row_at`): the table's rows, and the cell its key coordinate was placed in"""

    def __init__(self, rows): self.rows, self.key = rows, None


class _PickKey(_Sym):
    """the key coordinate of a pick: the index value itself"""

    def __init__(self, pick, inner): self.pick, self.inner = pick, inner


class _Gathered(_Sym):
    """coordinate t of the table row the pick's key names"""

    def __init__(self, pick, t): self.pick, self.t = pick, t


class _Segment:
    """one sort (`BaseRegion._sorted`): its source cells, its mode, and the cells its sorted values / their positions were placed in"""

    def __init__(self, src, mode):
        self.src, self.mode = src, mode
        self.dst = {SORT: [None] * len(src), ARGSORT: [None] * len(src)}


class _Sorted(_Sym):
    """the i-th smallest value of a segment"""
    kind = SORT

    def __init__(self, seg, i): self.seg, self.i = seg, i


class _SortedIndex(_Sorted):
    """the position in its segment of the i-th smallest value"""
    kind = ARGSORT


class _ArgExt(_Sym):
    """the position of the extremum of a segment (`BaseRegion._arg_extremum`): its source cells and its mode (0: max, 1: min)"""

    def __init__(self, src, mode): self.src, self.mode = src, mode


class _ScatterJob:
    """one scatter (`BaseRegion._scattered`): its base, index and source cells, the extent and multiplier of the scattered dimension, the
    constant offset of every element, and the cells its claim was placed in"""

    def __init__(self, base, index, src, extent, mult, offsets):
        self.base, self.index, self.src, self.extent, self.mult, self.offsets = base, index, src, extent, mult, offsets
        self.dst = [None] * len(base)


class _Scattered(_Sym):
    """element i of a scattered tensor"""

    def __init__(self, job, i): self.job, self.i = job, i


class _ComplementJob:
    """one missing set (`BaseRegion._missing`) over the positions 0 .. n - 1: its source cells and the cells its claim was placed in"""

    def __init__(self, n, src):
        self.n, self.src, self.dst = n, src, [None] * (n - len(src))


class _Missing(_Sym):
    """the i-th smallest position no source names"""

    def __init__(self, job, i): self.job, self.i = job, i


class _OneHot(_Sym):
    """entry `pos` of the one-hot vector of the index in cell a over `classes` (`BaseRegion._one_hot`)"""

    def __init__(self, a, pos, classes): self.a, self.pos, self.classes = a, pos, classes


class _Cmp(_Sym):
    def __init__(self, a, op, c):
        assert c == 0
        self.a, self.op = a, op
    def __sub__(self, o):                          # (s > 0) - (s < 0)
        assert isinstance(o, _Cmp) and self.op == ">" and o.op == "<" and o.a is self.a
        return _Sign(self.a)


class _Sign(_Sym):
    def __init__(self, a): self.a = a.idx
    def __mul__(self, o):                          # sgn(s) * ((|s| + d // 2) // d): round_div
        if not (isinstance(o, _MagDiv) and o.half is not None and o.mag.a == self.a):
            self._no()
        return _Div(self.a, o.div, o.mag.bound)


class _Mag(_Sym):
    """|signed value|; `mag < base ** legs` is the layout's range assertion: it is recorded, and checked at run time"""

    def __init__(self, a): self.a, self.bound = a.idx, None
    def __floordiv__(self, d): return _MagDiv(self, d)
    def __add__(self, half): return _MagHalf(self, half)
    def __lt__(self, bound):
        self.bound = bound
        return True


class _MagHalf(_Sym):
    """|x| + d // 2, then `// d`: the magnitude of a rounded quotient"""

    def __init__(self, mag, half): self.mag, self.half = mag, half
    def __floordiv__(self, d):
        if self.half != d // 2:
            self._no()
        return _MagDiv(self.mag, d, half=self.half)


class _MagDiv(_Sym):
    """|x| // base^e, then `% base`: a digit; with `half`, (|x| + d // 2) // d"""

    def __init__(self, mag, div, base=None, half=None): self.mag, self.div, self.base, self.half = mag, div, base, half
    def __mod__(self, m):
        if self.base is None:
            return _MagDiv(self.mag, self.div, m)
        assert m == R
        return self


class _Div(_Sym):
    """the signed value of cell a over the constant d, rounded half away from zero"""

    def __init__(self, a, d, bound): self.a, self.d, self.bound = a, d, bound


class _Shift(_Sym):
    """signed value - lo, |.| // col_size: the table-column index of a range check; without the |.|: that of a static lookup"""

    def __init__(self, a, lo): self.a, self.lo, self.absd, self.col_size = a.idx, lo, False, None
    def __abs__(self):
        self.absd = True
        return self
    def __floordiv__(self, c):
        self.col_size = c
        return self


class _Looked(_Sym):
    """table.f(signed value): the output of a static lookup"""

    def __init__(self, cell, table): self.cell, self.table = cell, table


def _ilog(x, base):
    e = 0
    while x > 1 and x % base == 0:
        x //= base
        e += 1
    if x != 1:
        raise PlanError("a digit divisor that is not a power of the base")
    return e


# ---- the recording region ----------------------------------------------------------------------------------------------------------------
class _Records:
    """cell writes grouped by kind and data dependence"""

    def __init__(self, earliest=False):
        self.recs = []                             # dict(kind, p0, p1, phase, dst, a, b) / for DOT: dict(kind, p0, dots) / for RLC: scans
        self.latest = {}                           # (kind, p0, p1, phase) -> record index
        self.of_key = {} if earliest else None     # earliest fit: (kind, p0, p1, phase) -> its record indices, ascending
        self.rec_of = {}                           # cell -> record that writes it

    def _new(self, key):
        self.recs.append(dict(kind=key[0], p0=key[1], p1=key[2], phase=key[-1], scalar=key[3] if len(key) == 5 else None, dst=[], a=[], b=[], dots=[], scans=[]))
        return len(self.recs) - 1

    def _slot(self, key, sources, phase=0, floor=0):
        key += (phase,)
        need = max(floor, 1 + max((self.rec_of[s] for s in sources), default=-1))     # floor: the record after which sources checked elsewhere are written
        if self.of_key is not None:                # the earliest record of the kind above every record the write reads from
            mine = self.of_key.setdefault(key, [])
            at = bisect.bisect_left(mine, need)
            if at < len(mine):
                return mine[at]
            mine.append(self._new(key))
            return mine[-1]
        ri = self.latest.get(key)
        if ri is None or ri < need:
            ri = self.latest[key] = self._new(key)
        return ri

    def _claim(self, dst, ri):
        if dst in self.rec_of:
            raise PlanError("advice cell %d is written twice: not a write-once layout" % dst)
        self.rec_of[dst] = ri

    def emit(self, kind, dst, a, b=None, p0=0, p1=0, reads=(), phase=0, floor=0):
        for s in reads:
            if s not in self.rec_of:
                raise PlanError("advice cell %d is read before it is written" % s)
        ri = self._slot((kind, p0, p1), reads, phase, floor)
        rec = self.recs[ri]
        rec["dst"].append(dst); rec["a"].append(a)
        if b is not None:
            rec["b"].append(b)
        self._claim(dst, ri)

    def emit_recip(self, dst, a, S, zero_inverse, phase=0):
        """one element of a RECIP record: the records are kept apart by S and by the constant a zero input takes (its index: the record's b)"""
        if a not in self.rec_of:
            raise PlanError("advice cell %d is read before it is written" % a)
        ri = self._slot((RECIP, S & NONE, S >> 32, zero_inverse), (a,), phase)
        rec = self.recs[ri]
        rec["dst"].append(dst); rec["a"].append(a)
        self._claim(dst, ri)

    def emit_dot(self, w, steps, phase=0):
        """steps: [(dst, [(a, b), ...])]"""
        reads = [c for _, pairs in steps for ab in pairs for c in ab]
        for s in reads:
            if s not in self.rec_of:
                raise PlanError("advice cell %d is read before it is written" % s)
        ri = self._slot((DOT, w, 0), reads, phase)
        self.recs[ri]["dots"].append(steps)
        for dst, _ in steps:
            self._claim(dst, ri)

    def emit_acc(self, kind, w, steps, phase=0):
        """one running sum / product: steps = [(dst, [cells])]"""
        reads = [c for _, cells in steps for c in cells]
        for s in reads:
            if s not in self.rec_of:
                raise PlanError("advice cell %d is read before it is written" % s)
        ri = self._slot((kind, w, 0), reads, phase)
        self.recs[ri]["scans"].append(steps)
        for dst, _ in steps:
            self._claim(dst, ri)

    def emit_sort(self, kind, mode, src, dst, phase=0):
        """one segment of a SORT / ARGSORT record: destination i gets the i-th smallest of the cells src (its value / its position)"""
        for s in src:
            if s not in self.rec_of:
                raise PlanError("advice cell %d is read before it is written" % s)
        ri = self._slot((kind, len(src), mode), src, phase)
        self.recs[ri]["scans"].append((list(src), list(dst)))
        for d in dst:
            self._claim(d, ri)

    def emit_argext(self, mode, src, dst, phase=0):
        """one segment of an ARGEXT record: the destination gets the position of the extremum of the cells src"""
        for s in src:
            if s not in self.rec_of:
                raise PlanError("advice cell %d is read before it is written" % s)
        ri = self._slot((ARGEXT, len(src), mode), src, phase)
        self.recs[ri]["scans"].append((list(src), dst))
        self._claim(dst, ri)

    def emit_scatter(self, job, phase=0):
        """a SCATTER record: one tensor, never shared"""
        reads = list(job.base) + list(job.index) + list(job.src)
        for s in reads:
            if s not in self.rec_of:
                raise PlanError("advice cell %d is read before it is written" % s)
        ri = self._new((SCATTER, len(job.index), job.mult, phase))
        self.recs[ri]["scans"].append(job)
        for d in job.dst:
            self._claim(d, ri)

    def emit_complement(self, job, phase=0):
        """a COMPLEMENT record: one set, never shared"""
        for s in job.src:
            if s not in self.rec_of:
                raise PlanError("advice cell %d is read before it is written" % s)
        ri = self._new((COMPLEMENT, job.n, len(job.src), phase))
        self.recs[ri]["scans"].append(job)
        for d in job.dst:
            self._claim(d, ri)

    def emit_scan(self, challenge, src, dst, phase):
        """one RLC scan: step t reads cell src[t] and writes cell dst[t]"""
        for s in src:
            if s not in self.rec_of:
                raise PlanError("advice cell %d is read before it is written" % s)
        ri = self._slot((RLC, challenge, len(src)), src, phase)
        self.recs[ri]["scans"].append((list(src), list(dst)))
        for d in dst:
            self._claim(d, ri)

    def emit_matmul(self, m, kd, n, a, b):
        """the record of an m x kd by kd x n integer product over the inputs a, b (row-major); its m * n destinations are claimed one by
        one (`matmul_dst`) as the layout places them"""
        ri = self._new((MATMUL, kd, n, 0))
        self.recs[ri].update(dst=[None] * (m * n), a=list(a), b=list(b))
        return ri

    def matmul_dst(self, ri, at, dst):
        if self.recs[ri]["dst"][at] is not None:
            raise PlanError("a matmul output is placed twice")
        self.recs[ri]["dst"][at] = dst
        self._claim(dst, ri)


class RecordingRegion(EL.BaseRegion):
    """BaseRegion with symbolic values: every placement decision is the parent's; `put` records how the cell is produced"""

    def __init__(self, gc, earliest=False):
        super().__init__(gc, witness=False)
        self.n_adv = len(gc.cs.advice)
        self.out = _Records(earliest)
        self.consts, self.const_idx = [], {}
        self.n_ops = 0
        self._dot = None

    def copy(self, a, b):                          # copy constraints belong to keygen, not to the witness
        pass

    def lookup_inputs_seen(self, signed_inputs):   # symbols have no extrema: the statistics of a replay are lookup_stats_host's
        pass

    def _const(self, v):
        v %= R
        if v not in self.const_idx:
            self.const_idx[v] = len(self.consts)
            self.consts.append(v)
        return self.const_idx[v]

    def put(self, var, linear, val):
        placed = super().put(var, linear, val)     # cell_of / cartesian_coord: the parent's placement
        _, col, row = placed.cell
        dst = (col << self.k) + row
        self._emit(val.v, dst)
        return EL.Val(_Cell(dst), placed.cell)

    def _emit(self, v, dst):
        out = self.out
        if isinstance(v, int):
            out.emit(CONST, dst, self._const(v))
        elif isinstance(v, _Cell):
            if self._dot is not None and self._dot and v.idx == self._dot[-1][0]:
                self._dot.append((dst, []))        # the running sum duplicated at the top of a new column: a step without products
            else:
                out.emit(COPY, dst, v.idx, reads=(v.idx,))
        elif isinstance(v, _Input):
            out.emit(INPUT, dst, v.idx)
        elif isinstance(v, _Param):
            out.emit(PARAM, dst, v.idx)
        elif isinstance(v, _Bin):
            out.emit(v.kind, dst, v.a, v.b, reads=(v.a, v.b))
        elif isinstance(v, _Un):
            out.emit(v.kind, dst, v.a, reads=(v.a,))
        elif isinstance(v, _Sign):
            base, legs = self._decomp
            out.emit(HINT, dst, v.a, NONE, p0=base, p1=legs, reads=(v.a,))
        elif isinstance(v, _Div):
            if v.bound != 1 << 52:
                raise PlanError("a division hint without the layout's range assertion")
            if not 1 <= v.d < 1 << 32:
                raise PlanError("a divisor beyond 32 bits")
            out.emit(DIVC, dst, v.a, p0=v.d, reads=(v.a,))
        elif isinstance(v, _MagDiv) and v.base is not None and v.half is None:
            base, legs = self._decomp
            if v.base != base or v.mag.bound != base ** legs:
                raise PlanError("a digit hint without the layout's range assertion")
            out.emit(HINT, dst, v.mag.a, _ilog(v.div, base), p0=base, p1=legs, reads=(v.mag.a,))
        elif isinstance(v, _Shift) and v.col_size is not None and v.absd:
            if not -(1 << 31) <= v.lo < 1 << 31 or not 0 < v.col_size < 1 << 32:
                raise PlanError("range check bounds beyond 32 bits")
            out.emit(RCIDX, dst, v.a, p0=v.lo & NONE, p1=v.col_size, reads=(v.a,))
        elif isinstance(v, _Acc):
            summed = [cell for cell, pairs in self._dot or [] if pairs]    # the steps so far, without the duplicated rows
            if self._dot is None or v.cell is not None or (v.prev is None) != (not summed) or (summed and v.prev.cell != summed[-1]):
                raise PlanError("a running sum outside the dot it belongs to")
            v.cell = dst
            self._dot.append((dst, v.pairs))
        else:
            raise PlanError("the witness plan recorder does not cover a %s value" % type(v).__name__)

    # ---- the ops: BaseRegion's own, counted; the out-of-scope ones refused by name -------------------------------------------------------
    def _counted(name):
        def op(self, *a, **kw):
            self.n_ops += 1
            return getattr(EL.BaseRegion, name)(self, *a, **kw)
        op.__name__ = name
        return op
    pairwise, enforce_equality, range_check = _counted("pairwise"), _counted("enforce_equality"), _counted("range_check")

    def decompose(self, vals, base, legs, zero_sign_matters=False):
        self.n_ops += 1
        self._decomp = (base, legs)
        if base ** legs >= 1 << 62:
            raise PlanError("decomposition range beyond 62 bits")
        return super().decompose(vals, base, legs, zero_sign_matters)

    def dot(self, a, b):
        self.n_ops += 1
        self._dot = []
        try:
            last = super().dot(a, b)
            steps = self._dot
        finally:
            self._dot = None
        self.out.emit_dot(self.w, steps)
        return last

    def _refused(name):
        def op(self, *a, **kw):
            raise PlanError("witness plans do not cover `%s` (the MLP op family only: decompose, range_check, dot, pairwise, "
                            "enforce_equality, equals_zero, relu, div, output_equals_instance)" % name)
        return op
    nonlinearity, sum, prod, _accumulate = _refused("nonlinearity"), _refused("sum"), _refused("prod"), _refused("sum / prod")
    dynamic_lookup, shuffle, _lookup_any = _refused("dynamic_lookup"), _refused("shuffle"), _refused("lookup_any")
    sort_ascending, topk, _sorted = _refused("sort_ascending"), _refused("topk"), _refused("sort_ascending")
    recip, sqrt, rsqrt, max, min = _refused("recip"), _refused("sqrt"), _refused("rsqrt"), _refused("max"), _refused("min")
    percent, softmax, softmax_axes, mean_of_squares = _refused("percent"), _refused("softmax"), _refused("softmax_axes"), _refused("mean_of_squares")
    select, argmax, argmin, argmax_axes, argmin_axes = _refused("select"), _refused("argmax"), _refused("argmin"), _refused("argmax_axes"), _refused("argmin_axes")
    max_pool, sumpool, _arg_extremum = _refused("max_pool"), _refused("sumpool"), _refused("argmax / argmin")
    select_elements, linearize_element_index, gather, gather_elements = _refused("select_elements"), _refused("linearize_element_index"), _refused("gather"), _refused("gather_elements")
    one_hot, one_hot_axis, _one_hot, shuffles, _claimed_indices = _refused("one_hot"), _refused("one_hot_axis"), _refused("one_hot"), _refused("shuffles"), _refused("shuffles")
    get_missing_set_elements, _missing = _refused("get_missing_set_elements"), _refused("get_missing_set_elements")
    scatter_elements, _scattered = _refused("scatter_elements"), _refused("scatter_elements")
    del _counted, _refused


def _table_values(table):
    """f over the table's range [lo, hi] as int64"""
    lo, hi = table.range
    if not (-(1 << 31) <= lo <= hi < 1 << 31) or not 0 < table.col_size < 1 << 32:
        raise PlanError("lookup table bounds beyond 32 bits")
    vals = [int(table.f(x)) for x in range(lo, hi + 1)]
    if any(not -(1 << 63) <= v < 1 << 63 for v in vals):
        raise PlanError("a lookup table value beyond int64")
    return np.array(vals, np.int64)


class _SymTable:
    """what BaseRegion.nonlinearity reads of a Table, with `f` answering a symbol"""

    def __init__(self, table, index):
        self.range, self.col_size, self.index = tuple(table.range), table.col_size, index

    def f(self, x):
        if not isinstance(x, _Cell):
            raise PlanError("a lookup on a %s value" % type(x).__name__)
        return _Looked(x, self)


class _SymBase:
    """the region's BaseConfig with the static tables replaced by their stand-ins (made on first use); everything else is the config's own"""

    def __init__(self, base, region):
        self._base, self.static_tables = base, _SymTables(base, region)

    def __getattr__(self, name):
        return getattr(self._base, name)


class _SymTables(dict):
    def __init__(self, base, region): self.base, self.region = base, region
    def __missing__(self, name):
        table = self.base.static_tables[name]
        self[name] = sym = _SymTable(table, len(self.region.tables))
        self.region.tables.append((table.range[0], table.col_size, _table_values(table)))
        return sym


class LookupRecordingRegion(RecordingRegion):
    """RecordingRegion + `nonlinearity` (a static lookup: TABLE for f(x), TBLIDX for the table column beside it), with records grouped by
    dependence level.  tables: [(lo, col_size, values as int64)] in order of first use."""

    def __init__(self, gc):
        super().__init__(gc, earliest=True)
        self.tables = []
        self.base = _SymBase(gc.base, self)
        self._lookup_src = {}                      # source cell -> (its symbol, table) of the lookups recorded so far
        self._scan = None                          # the steps of the `sum` / `prod` being laid out
        self.gather_tables, self._gather_idx = [], {}     # the cell lists GATHER records index, in order of first use
        self._keyed_rows = None                           # the table whose keys `row_at` has found to be its positions: the latest one
        self._gather_of = (None, None, None, 0)           # (the placed table, the coordinate, its cells, the record after them) of the latest pick
        self.param_values = None                   # record_plan's parameter list: what a _Param stands for

    def nonlinearity(self, vals, name):
        self.n_ops += 1
        return EL.BaseRegion.nonlinearity(self, vals, name)

    # ---- sum / prod: BaseRegion._accumulate on symbols -> one SUMACC / PRODACC scan ----------------------------------------------------------
    sum, prod = EL.BaseRegion.sum, EL.BaseRegion.prod

    def _accumulate(self, vals, init_op, op, unit, fold):
        self.n_ops += 1
        self._scan = []
        try:
            last = EL.BaseRegion._accumulate(self, vals, init_op, op, unit, fold)
            steps = self._scan
        finally:
            self._scan = None
        kinds = {kind for _, _, kind in steps if kind is not None}
        if kinds != {SUMACC if unit == 0 else PRODACC}:
            raise PlanError("a running value of another fold than its op's")
        self.out.emit_acc(kinds.pop(), self.w, [(dst, cells) for dst, cells, _ in steps])
        return last

    # ---- dynamic_lookup / shuffle: both sides are placed through `put` (BaseRegion._lookup_any) ------------------------------------------------
    _lookup_any = EL.BaseRegion._lookup_any

    def dynamic_lookup(self, table_rows, picks):
        self.n_ops += 1
        return EL.BaseRegion.dynamic_lookup(self, table_rows, picks)

    def shuffle(self, rows, order):
        self.n_ops += 1
        if not all(isinstance(i, (int, np.integer)) for i in order):
            raise PlanError("witness plans do not cover `shuffle` with a data-dependent order (sort, top-k): the order must be integers")
        return EL.BaseRegion.shuffle(self, rows, order)

    # ---- sort / top-k: BaseRegion's ops around `_sorted` ----------------------------------------------------------------------------------------
    def sort_ascending(self, vals, mode="unsorted"):
        self.n_ops += 1
        return EL.BaseRegion.sort_ascending(self, vals, mode)

    topk = EL.BaseRegion.topk

    # ---- recip / sqrt and what is built on them: BaseRegion's ops around `recip_claim` / `sqrt_claim` ----------------------------------------------
    def recip(self, vals, input_scale, output_scale, eps):
        self.n_ops += 1
        return EL.BaseRegion.recip(self, vals, input_scale, output_scale, eps)

    def sqrt(self, vals, input_scale):
        self.n_ops += 1
        return EL.BaseRegion.sqrt(self, vals, input_scale)

    rsqrt, max, min, percent = EL.BaseRegion.rsqrt, EL.BaseRegion.max, EL.BaseRegion.min, EL.BaseRegion.percent
    softmax, softmax_axes, mean_of_squares = EL.BaseRegion.softmax, EL.BaseRegion.softmax_axes, EL.BaseRegion.mean_of_squares

    # ---- argmax / argmin and the pooling ops: BaseRegion's ops around `_arg_extremum` -------------------------------------------------------------
    def argmax(self, vals):
        self.n_ops += 1
        return EL.BaseRegion.argmax(self, vals)

    def argmin(self, vals):
        self.n_ops += 1
        return EL.BaseRegion.argmin(self, vals)

    select, argmax_axes, argmin_axes = EL.BaseRegion.select, EL.BaseRegion.argmax_axes, EL.BaseRegion.argmin_axes
    max_pool, sumpool = EL.BaseRegion.max_pool, EL.BaseRegion.sumpool

    # ---- gather / scatter / one-hot: BaseRegion's ops around `_scattered`, `_missing`, `_one_hot` and `_claimed_indices` ------------------------------
    def scatter_elements(self, input, dims, index, index_dims, src, dim):
        self.n_ops += 1
        return EL.BaseRegion.scatter_elements(self, input, dims, index, index_dims, src, dim)

    def one_hot(self, index, num_classes):
        self.n_ops += 1
        if not isinstance(index.v, _Cell):                # (`signed` of any other symbol is refused without a name)
            raise PlanError("a one-hot over an index that is not an assigned cell")
        return EL.BaseRegion.one_hot(self, index, num_classes)

    def gather(self, vals, dims, index, dim):
        self.n_ops += 1
        return EL.BaseRegion.gather(self, vals, dims, index, dim)

    def gather_elements(self, vals, dims, index, index_dims, dim):
        self.n_ops += 1
        return EL.BaseRegion.gather_elements(self, vals, dims, index, index_dims, dim)

    def get_missing_set_elements(self, vals, fullset, ordered):
        self.n_ops += 1
        return EL.BaseRegion.get_missing_set_elements(self, vals, fullset, ordered)

    select_elements, linearize_element_index, one_hot_axis, shuffles = (EL.BaseRegion.select_elements, EL.BaseRegion.linearize_element_index,
                                                                         EL.BaseRegion.one_hot_axis, EL.BaseRegion.shuffles)

    @staticmethod
    def _cells_of(vals, what):
        if not all(isinstance(v.v, _Cell) for v in vals):
            raise PlanError("%s over values that are not assigned cells" % what)
        return [v.v.idx for v in vals]

    def _positions(self, fullset):
        """True when the full set is the constants 0 .. n - 1 in order"""
        return all(v.const and isinstance(v.v, (int, np.integer)) and v.v == j for j, v in enumerate(fullset))

    def _scattered(self, input, index, src, dims, index_dims, dim):
        """BaseRegion._scattered on symbols: one SCATTER record over the cells the base, the index and the source are assigned in, emitted
        once the layout has placed the whole claim"""
        assert len(index) == len(src) and all(a <= b for t, (a, b) in enumerate(zip(index_dims, dims)) if t != dim)
        mult = self._strides(dims)
        offsets = [sum(coord[t] * mult[t] for t in range(len(dims)) if t != dim) for coord in self._coords(index_dims)]
        job = _ScatterJob(self._cells_of(input, "a scatter"), self._cells_of(index, "a scatter"), self._cells_of(src, "a scatter"), dims[dim], mult[dim], offsets)
        return [_Scattered(job, i) for i in range(len(input))]

    def _missing(self, vals, fullset):
        """BaseRegion._missing on symbols: one COMPLEMENT record over the cells the values are assigned in; the full set must be the
        positions"""
        if not self._positions(fullset):
            raise PlanError("a missing-set over a full set that is not the positions 0 .. n - 1")
        if len(vals) > len(fullset):
            raise PlanError("a missing-set of more values than the full set holds")
        job = _ComplementJob(len(fullset), self._cells_of(vals, "a missing-set"))
        return [_Missing(job, i) for i in range(len(job.dst))]

    def _one_hot(self, s, num_classes):
        """BaseRegion._one_hot on the symbol of the index's signed value: ONEHOT elements"""
        if not isinstance(s, _Cell):
            raise PlanError("a one-hot over an index that is not an assigned cell")
        if not 1 <= num_classes < 1 << 32:
            raise PlanError("one-hot classes outside [1, 2^32)")
        return [_OneHot(s, j, num_classes) for j in range(num_classes)]

    def _claimed_indices(self, output, input):
        """BaseRegion._claimed_indices on symbols: over the positions 0 .. n - 1 the first unused position that holds an output element's value
        is that value itself -- a COPY of the element's cell"""
        if not self._positions(input):
            raise PlanError("a missing-set over a full set that is not the positions 0 .. n - 1")
        self._cells_of(output, "a permutation argument")
        return [v.v for v in output]

    def _arg_extremum(self, vals, mode):
        """BaseRegion._arg_extremum on symbols: one segment of an ARGEXT record over the cells the values are assigned in, emitted when the
        layout places the claim"""
        if not all(isinstance(v.v, _Cell) for v in vals):
            raise PlanError("an arg-extremum over values that are not assigned cells")
        return _ArgExt([v.v.idx for v in vals], {"max": 0, "min": 1}[mode])

    def _sorted(self, vals, mode):
        """BaseRegion._sorted on symbols: one segment over the cells the values are assigned in; its sorted values and their positions are
        collected as the layout places them and emitted, each list as one segment, once it is whole"""
        if not all(isinstance(v.v, _Cell) for v in vals):
            raise PlanError("a sort over values that are not assigned cells")
        seg = _Segment([v.v.idx for v in vals], int(mode == "largest_index_first"))
        return [_Sorted(seg, i) for i in range(len(vals))], [_SortedIndex(seg, i) for i in range(len(vals))]

    def row_at(self, table_rows, index):
        """BaseRegion.row_at on symbols: the key coordinate is the index value itself, every other coordinate a GATHER element over the
        cells of the dynamic table the pick is looked up in -- which must be this very list, with the positions 0 .. n - 1 as its keys"""
        for r, row in enumerate(() if table_rows is self._keyed_rows else table_rows):     # (the picks of one lookup share the list: checked once)
            key = row[0].v if isinstance(row[0], EL.Val) else row[0]
            if isinstance(key, _Param) and self.param_values is not None:
                key = self.param_values[key.idx]
            if not isinstance(key, (int, np.integer)) or key % R != r:
                raise PlanError("a gather over a table whose keys are not its positions")
        self._keyed_rows = table_rows
        if not isinstance(index.v, (_Input, _Cell)):
            raise PlanError("a gather index that is a %s value" % type(index.v).__name__)
        pick = _Pick(table_rows)
        return (EL.Val(_PickKey(pick, index.v)),) + tuple(EL.Val(_Gathered(pick, t)) for t in range(1, len(table_rows[0])))

    def _asserted(self, cell, table):
        if (getattr(cell, "lo", None), getattr(cell, "hi", None)) != table.range:
            raise PlanError("a lookup without the layout's range assertion")

    def _emit(self, v, dst):
        if self._scan is not None and isinstance(v, _Cell) and self._scan and v.idx == self._scan[-1][0]:
            self._scan.append((dst, [], None))     # the running value duplicated at the top of a new column: a step without operands
        elif isinstance(v, _Fold):
            folded = [cell for cell, cells, _ in self._scan or [] if cells]
            if self._scan is None or v.cell is not None or (v.prev is None) != (not folded) or (folded and v.prev.cell != folded[-1]):
                raise PlanError("a running value outside the sum / prod it belongs to")
            v.cell = dst
            self._scan.append((dst, v.cells, v.kind))
        elif isinstance(v, _Sorted):
            placed = v.seg.dst[v.kind]
            if placed[v.i] is not None:
                raise PlanError("a sorted value is placed twice")
            placed[v.i] = dst
            if None not in placed:
                self.out.emit_sort(v.kind, v.seg.mode, v.seg.src, placed)
        elif isinstance(v, _ArgExt):
            self.out.emit_argext(v.mode, v.src, dst)
        elif isinstance(v, (_Scattered, _Missing)):
            placed = v.job.dst
            if placed[v.i] is not None:
                raise PlanError("a claimed element is placed twice")
            placed[v.i] = dst
            if None not in placed:
                (self.out.emit_scatter if isinstance(v, _Scattered) else self.out.emit_complement)(v.job)
        elif isinstance(v, _OneHot):
            self.out.emit(ONEHOT, dst, v.a.idx, v.pos, p0=v.classes, reads=(v.a.idx,))
        elif isinstance(v, _Clamp):
            if not -(1 << 31) <= v.lo <= v.hi < 1 << 31:
                raise PlanError("clamp bounds beyond 32 bits")
            self.out.emit(CLAMP, dst, v.a, p0=v.lo & NONE, p1=v.hi & NONE, reads=(v.a,))
        elif isinstance(v, _Recip):
            if not 1 <= v.S < 1 << 62:
                raise PlanError("a reciprocal at a scale outside [1, 2^62)")
            self.out.emit_recip(dst, v.a, v.S, self._const(v.zero_inverse))
        elif isinstance(v, _Isqrt):
            if not 1 <= v.scale < 1 << 32:
                raise PlanError("a square root at a scale outside [1, 2^32)")
            self.out.emit(ISQRT, dst, v.a, p0=v.scale, reads=(v.a,))
        elif isinstance(v, _PickKey):
            self._emit(v.inner, dst)
            v.pick.key = dst
        elif isinstance(v, _Gathered):
            rows, placed = getattr(self, "dyn_table", (None, None))
            if rows is not v.pick.rows or v.pick.key is None:
                raise PlanError("a gather pick outside the dynamic lookup over its table")
            if self._gather_of[0] is not placed or self._gather_of[1] != v.t:       # the picks of one lookup share the table: its cells are listed, and looked up, once
                cells = tuple(placed[r][v.t].v.idx for r in range(len(rows)))
                for c in cells:
                    if c not in self.out.rec_of:
                        raise PlanError("advice cell %d is read before it is written" % c)
                if cells not in self._gather_idx:
                    self._gather_idx[cells] = len(self.gather_tables)
                    self.gather_tables.append(cells)
                self._gather_of = (placed, v.t, cells, 1 + max(self.out.rec_of[c] for c in cells))
            _, _, cells, floor = self._gather_of
            self.out.emit(GATHER, dst, v.pick.key, p0=self._gather_idx[cells], p1=len(cells), reads=(v.pick.key,), floor=floor)
        elif isinstance(v, _Looked):
            self._asserted(v.cell, v.table)
            self._lookup_src[v.cell.idx] = (v.cell, v.table)
            self.out.emit(TABLE, dst, v.cell.idx, p0=v.table.index, reads=(v.cell.idx,))
        elif isinstance(v, _Shift) and v.col_size is not None and not v.absd:
            src = self._lookup_src.get(v.a)
            if src is None or v.lo != src[1].range[0] or v.col_size != src[1].col_size:
                raise PlanError("a table-column index without its lookup")
            self._asserted(*src)
            self.out.emit(TBLIDX, dst, v.a, p0=src[1].index, reads=(v.a,))
        else:
            super()._emit(v, dst)


class _MatOut(_Sym):
    """entry `at` of the integer product of matmul record `rec`"""

    def __init__(self, rec, at): self.rec, self.at = rec, at


class _Placed(_Sym):
    """a value whose cell is fixed before the layout reaches it -- an element of an einsum's claimed product, whose DOT record is emitted
    ahead of the layout -- : `put_cell` only checks that the layout places it there"""

    def __init__(self, dst): self.dst = dst


class _Tag(_Sym):
    """what a layout pass that only asks WHERE things land carries as a value (`_Probe`)"""

    def __init__(self, key=None): self.key = key


class _Probe(EL.Region):
    """a Region that records, for every tagged value, the first cell the layout places it in: no cells, selectors or copies"""

    def __init__(self, cs, k, coord):
        super().__init__(cs, k)
        self.coord, self.where = coord, {}

    def copy(self, a, b): pass
    def enable(self, selector, row): pass
    def constant(self, const_cols, value): return None

    def put_cell(self, col, row, v):
        if isinstance(v, _Tag) and v.key is not None:
            self.where.setdefault(v.key, (col, row))
        return v

    tagged = staticmethod(lambda xs, *_: [EL.Val(_Tag()) for _ in xs])
    rlc = dot = sum = prod = mul = tagged


class _Run:
    """the running values of one RLC scan, one dot or one running sum / product, pending until the layout has placed every step"""

    def __init__(self, kind, p0, src): self.kind, self.p0, self.src, self.dst, self.left = kind, p0, src, [None] * len(src), len(src)


class _Step(_Sym):
    def __init__(self, run, t): self.run, self.t = run, t


class _EinsumOps:
    """what EinsumCircuit.sequence asks of its `ops`, answered by an EinsumRecordingRegion's symbols (by the class's own methods: on a
    PhasedLookupRecordingRegion `dot` and `sum` are the model's ops)"""

    def __init__(self, reg): self.reg = reg
    def rlc(self, vals, ci): return EinsumRecordingRegion.rlc(self.reg, vals, ci)
    def dot(self, xs, ys): return EinsumRecordingRegion.dot(self.reg, xs, ys)
    def sum(self, xs): return EinsumRecordingRegion.acc(self.reg, SUMACC, xs)
    def prod(self, xs): return EinsumRecordingRegion.acc(self.reg, PRODACC, xs)
    def mul(self, xs, ys): return EinsumRecordingRegion.mul(self.reg, xs, ys)


class EinsumRecordingRegion(EL.Region):
    """Region with symbolic values for EinsumMatmulCircuit.sequence: the rows are those `_assign` computes from the shared coordinate,
    `put_cell` records how the cell is produced and in which phase -- phase 0 for inputs and the integer product, at least 1 for
    whatever a challenge enters, otherwise the latest phase among the cells read -- and refuses a value placed in a column of another
    phase.  Records are grouped by kind, phase and dependence level."""

    def __init__(self, circuit, k=None):
        cs, k = (circuit.cs, circuit.k) if k is None else (circuit, k)     # a circuit, or -- as Region -- its constraint system and k
        super().__init__(cs, k)
        self.n_adv = len(cs.advice)
        self.out = _Records(earliest=True)
        self.consts, self.n_ops = [], 0
        self.phase_of = {}                         # cell -> the phase that writes it
        self.preplaced = {}                        # cell -> the operand symbol an einsum's claim had placed there ahead of the layout

    def copy(self, a, b):                          # copy constraints and selectors belong to keygen, not to the witness
        pass

    def enable(self, selector, row):
        pass

    def matmul(self, m, kd, n, a, b):
        self.n_ops += 1
        ri = self.out.emit_matmul(m, kd, n, a, b)
        return [EL.Val(_MatOut(ri, at)) for at in range(m * n)]

    def _cells(self, vals):
        if not all(isinstance(v.v, _Cell) for v in vals):
            raise PlanError("a reduction over values that are not assigned cells")
        return [v.v.idx for v in vals]

    def rlc(self, vals, challenge):
        self.n_ops += 1
        run = _Run(RLC, challenge, self._cells(vals))
        return [EL.Val(_Step(run, t)) for t in range(len(vals))]

    def dot(self, xs, ys):
        self.n_ops += 1
        run = _Run(DOT, 1, list(zip(self._cells(xs), self._cells(ys))))
        return [EL.Val(_Step(run, t)) for t in range(len(xs))]

    def acc(self, kind, xs):
        """the running values of the einsum's `sum` (SUMACC) or `prod` (PRODACC): one scan of one operand per step"""
        run = _Run(kind, 1, self._cells(xs))
        return [EL.Val(_Step(run, t)) for t in range(len(xs))]

    def mul(self, xs, ys):
        return [EL.Val(_Bin(MUL, x.v, y.v)) for x, y in zip(xs, ys)]

    def lay_einsum(self, ein, operands):
        """an EinsumCircuit's `sequence` over symbols.  The prover's claim -- the product -- is ONE DOT record in phase 0: count = |O| dots
        of one step (p1 = 1) of p0 = K products, K the index tuples of the axes that are not in the output (an operand without such an
        axis repeats its cell); pool cost 2 * K * |O| words.  It reads CELLS: the cell an operand element already holds, else the
        first-phase einsum cell its own input reduction places it in.  The layout writes the claim BEFORE those cells, and a record
        reads only cells of earlier records: so the einsum is laid out once on a `_Probe` to learn where the operands and the product
        land, the operand cells are placed ahead of the layout, the claim is emitted, and the layout then finds both where it puts
        them.  Returns the product as Vals that carry the claimed cells."""
        import itertools, math
        self.n_ops += 1
        an, dims = ein.analysis, ein.dims
        contracted = sorted(set("".join(ein.exprs)) - set(an.output_indices))
        K, n_out = math.prod(dims[c] for c in contracted), math.prod(ein.out_shape)
        if 2 * K * n_out > MAX_CLAIM_WORDS:
            raise PlanError(CLAIM_ERROR)
        probe = _Probe(self.cs, self.k, self.coord)
        ein.sequence(probe, [[EL.Val(_Tag(("operand", t, e))) for e in range(len(vals))] for t, vals in enumerate(operands)],
                     [EL.Val(_Tag(("product", at))) for at in range(n_out)], probe, 1)
        cells = []
        for t, vals in enumerate(operands):
            mine = []
            for e, val in enumerate(vals):
                if isinstance(val.v, _Cell):                       # a cell the circuit computed: read where it is
                    mine.append(val.v.idx)
                    continue
                col, row = probe.where[("operand", t, e)]
                if self.cs.advice[col.index].phase != 0:
                    raise PlanError("an einsum operand that starts outside the first phase")
                mine.append(self.put_cell(col, row, val.v).idx)
                self.preplaced[mine[-1]] = val.v
            cells.append(mine)
        strides = [dict(zip(e, ein._strides([dims[c] for c in e]))) for e in ein.exprs]
        ri = self.out._new((DOT, K, 0, 0))
        product = []
        for at, out_pos in enumerate(itertools.product(*[range(n) for n in ein.out_shape])):
            pos = dict(zip(an.output_indices, out_pos))
            pairs = []
            for inner in itertools.product(*[range(dims[c]) for c in contracted]):
                pos.update(zip(contracted, inner))
                pairs.append(tuple(cells[t][sum(pos[c] * strides[t][c] for c in ein.exprs[t])] for t in (0, 1)))
            col, row = probe.where[("product", at)]
            dst = (col.index << self.k) + row
            for c in (c for ab in pairs for c in ab):
                if c not in self.out.rec_of:
                    raise PlanError("advice cell %d is read before it is written" % c)
            self.out.recs[ri]["dots"].append([(dst, pairs)])
            self.out._claim(dst, ri)
            if self.cs.advice[col.index].phase != 0 or dst in self.phase_of:
                raise PlanError("an einsum's claim outside a free first-phase cell")
            self.phase_of[dst] = 0
            product.append(EL.Val(_Placed(dst)))
        return ein.sequence(self, operands, product, _EinsumOps(self), 1)

    def put_cell(self, col, row, v):
        dst = (col.index << self.k) + row
        out = self.out
        if isinstance(v, _Placed):
            if v.dst != dst:
                raise PlanError("a claimed product element is placed in another cell than its claim names")
            return _Cell(dst)
        if dst in self.preplaced and self.preplaced[dst] is v:
            del self.preplaced[dst]
            return _Cell(dst)
        if isinstance(v, _Input):
            phase = 0
            out.emit(INPUT, dst, v.idx)
        elif isinstance(v, _Param):
            phase = 0
            out.emit(PARAM, dst, v.idx)
        elif isinstance(v, _Bin):
            phase = max(self.phase_of[v.a], self.phase_of[v.b])
            out.emit(v.kind, dst, v.a, v.b, reads=(v.a, v.b), phase=phase)
        elif isinstance(v, _MatOut):
            phase = 0
            out.matmul_dst(v.rec, v.at, dst)
        elif isinstance(v, _Cell):
            phase = self.phase_of[v.idx]
            out.emit(COPY, dst, v.idx, reads=(v.idx,), phase=phase)
        elif isinstance(v, _Step):
            run = v.run
            if run.dst[v.t] is not None:
                raise PlanError("a running value is placed twice")
            run.dst[v.t] = dst
            run.left -= 1
            if run.left == len(run.src) - 1:       # the phase of the whole run: worked out once, at its first step
                run.phase = max([1 if run.kind == RLC else 0] + [self.phase_of[c] for c in (run.src if run.kind != DOT else [c for ab in run.src for c in ab])])
            phase = run.phase
            if run.kind == RLC:
                if not run.left:
                    out.emit_scan(run.p0, run.src, run.dst, phase)
            elif run.kind in (SUMACC, PRODACC):
                if not run.left:
                    out.emit_acc(run.kind, run.p0, [(d, [c]) for d, c in zip(run.dst, run.src)], phase)
            else:
                if not run.left:
                    out.emit_dot(run.p0, [(d, [ab]) for d, ab in zip(run.dst, run.src)], phase)
        else:
            raise PlanError("the witness plan recorder does not cover a %s value in an einsum" % type(v).__name__)
        if phase != self.cs.advice[col.index].phase:
            raise PlanError("advice column %d belongs to phase %d, the value placed in it to phase %d" % (col.index, self.cs.advice[col.index].phase, phase))
        if dst in self.phase_of:
            raise PlanError("advice cell %d is written twice: not a write-once layout" % dst)
        self.phase_of[dst] = phase
        return _Cell(dst)


class PhasedLookupRecordingRegion(LookupRecordingRegion, EinsumRecordingRegion):
    """LookupRecordingRegion for a circuit that lays an einsum over its own configuration (`BaseRegion.einsum`): the model ops are
    placed by `put` (phase 0), the einsum's cells by EinsumRecordingRegion's `put_cell` with its matmul record, running values and phase
    bookkeeping -- one record list, one cell numbering.  (The constructor chain ends in EinsumRecordingRegion's, as a Region's.)"""

    def put(self, var, linear, val):
        placed = super().put(var, linear, val)
        dst = placed.v.idx
        if self.cs.advice[dst >> self.k].phase != 0:
            raise PlanError("advice column %d belongs to phase %d, the model op placed in it to phase 0" % (dst >> self.k, self.cs.advice[dst >> self.k].phase))
        self.phase_of[dst] = 0
        return placed

    def einsum(self, ein, A, B, challenges=None):
        if isinstance(ein, EL.EinsumCircuit):
            return [EL.Val(v.v, ("adv", v.v.idx >> self.k, v.v.idx & ((1 << self.k) - 1))) for v in self.lay_einsum(ein, [list(A), list(B)])]
        L = ein.len
        flat = [v.v for M in (A, B) for row in M for v in row]
        if not all(isinstance(v, _Input) for v in flat):
            raise PlanError("an einsum over operands that are not model inputs")
        O = self.matmul(L, L, L, [v.idx for v in flat[:L * L]], [v.idx for v in flat[L * L:]])
        ein.sequence(self, A, B, O, self.rlc, lambda xs, ys: EinsumRecordingRegion.dot(self, xs, ys), 1)


def _record_einsum(circuit):
    """EinsumMatmulCircuit: its own `sequence` over symbols -- the inputs are A then B, row-major; the product is one MATMUL record"""
    L = circuit.len
    if (len(circuit.cs.advice) << circuit.k) > 1 << 32:
        raise PlanError("cells are numbered in 32 bits")
    reg = EinsumRecordingRegion(circuit)
    Val = EL.Val
    A = [[Val(_Input(i * L + j)) for j in range(L)] for i in range(L)]
    B = [[Val(_Input(L * L + j * L + kk)) for kk in range(L)] for j in range(L)]
    O = reg.matmul(L, L, L, range(L * L), range(L * L, 2 * L * L))
    reg.out._slot((INPUT, 0, 0), ())               # the input record next: it reads no cell, and a reduction over inputs can then join the earliest of its kind
    circuit.sequence(reg, A, B, O, reg.rlc, reg.dot, 1)
    return WitnessPlan._from_recorder(circuit, reg, [], [], n_challenges=len(circuit.cs.challenges),
                                      n_phases=1 + max(c.phase for c in circuit.cs.advice))


def _record_general_einsum(circuit):
    """a standalone EinsumCircuit: its own `sequence` over symbols (EinsumRecordingRegion.lay_einsum) -- the inputs are the first operand,
    then the second, row-major; the product is one DOT record over their cells"""
    if (len(circuit.cs.advice) << circuit.k) > 1 << 32:
        raise PlanError("cells are numbered in 32 bits")
    reg = EinsumRecordingRegion(circuit)
    at = [0, circuit.sizes[0]]
    reg.lay_einsum(circuit, [[EL.Val(_Input(at[t] + e)) for e in range(circuit.sizes[t])] for t in (0, 1)])
    return WitnessPlan._from_recorder(circuit, reg, [], [], n_challenges=len(circuit.cs.challenges),
                                      n_phases=1 + max(c.phase for c in circuit.cs.advice))


def params_hash(circuit):
    """what a plan depends on besides the layout code: the circuit's `plan_identity()` bytes -- its shape options and its parameters -- and
    its static lookup tables, where its class has them hashed in (`plan_tables`).  The domain prefix is the class's `plan_domain`, by
    default b"layout:<ClassName>:" (none for an MlpCircuit, whose hashes stay what they were).
    An MlpCircuit's identity takes its visibility triple in unless it is the default one: the module columns of a KZG-committed tensor, the
    instance-fed cells of a public input and the constants of Fixed parameters are INPUT / PARAM / CONST / COPY records of another plan,
    and a `.wplan` written for another triple next to a key is recorded again, not replayed."""
    h = hashlib.sha256(_plan_domain(circuit) + circuit.plan_identity())
    for name, table in sorted(circuit.gc.base.static_tables.items()) if getattr(circuit, "plan_tables", True) else ():
        h.update(name.encode() + struct.pack("<3q", table.range[0], table.range[1], table.col_size))
        h.update(_table_values(table).tobytes())
    return h.digest()


def _plan_domain(circuit):
    domain = getattr(circuit, "plan_domain", None)
    return ("layout:%s:" % type(circuit).__name__).encode() if domain is None else domain


_STANDALONE_RECORDERS = {b"phased:": _record_einsum, b"einsum:": _record_general_einsum}


def record_plan(circuit):
    """one witness-free layout pass -> WitnessPlan, with the input vector and the parameters as symbols.  A circuit built on BaseRegion
    states its op sequence itself -- `layout(reg, inputs, param) -> outputs`, which its own `synthesize` runs too, with `n_inputs` and
    `plan_identity()` (MlpCircuit, ConvMnistCircuit) -- and is recorded from that; the parameters enter the blob in the order `layout` asks
    for them.  Only the recording region is chosen here, by what the circuit's class declares (ezkl_layout.LayoutCircuit): the one without a
    domain prefix, MlpCircuit, keeps RecordingRegion (latest-fit grouping, `nonlinearity` refused by name: its blobs stay what they
    were); one that declares `lays_einsums` -- second-phase advice of its own; such columns without the declaration are refused -- gets
    a PhasedLookupRecordingRegion and a plan with phases; any other a LookupRecordingRegion.  An EinsumMatmulCircuit or EinsumCircuit
    with columns of its own (not one laid over another circuit's) is recorded from its `sequence` into a two-phase plan.  Every other
    circuit class is refused by name."""
    standalone = _STANDALONE_RECORDERS.get(_plan_domain(circuit))
    if standalone is not None and getattr(circuit, "standalone", False):
        return standalone(circuit)
    if not (callable(getattr(circuit, "layout", None)) and callable(getattr(circuit, "plan_identity", None))):
        raise PlanError("witness plans cover MlpCircuit and circuits that state their `layout`, not %s" % type(circuit).__name__)
    if getattr(circuit, "gc", None) is None:
        raise PlanError("witness plans are recorded from a configured circuit: this %s has no configuration" % type(circuit).__name__)
    phased = any(c.phase != 0 for c in circuit.gc.cs.advice)                    # einsums laid over its own configuration: a two-phase plan
    if phased and not getattr(circuit, "lays_einsums", False):
        raise PlanError("witness plans do not cover second-phase advice")
    reg = (RecordingRegion if _plan_domain(circuit) == b"" else PhasedLookupRecordingRegion if phased else LookupRecordingRegion)(circuit.gc)
    if (len(circuit.gc.cs.advice) << circuit.k) > 1 << 32:
        raise PlanError("cells are numbered in 32 bits")
    params = []
    def param(v):
        v = int(v)
        if not -(1 << 63) <= v < 1 << 63:
            raise PlanError("a parameter beyond int64")
        params.append(v)
        return EL.Val(_Param(len(params) - 1))
    reg.param_values = params
    outs = circuit.layout(reg, [EL.Val(_Input(i)) for i in range(circuit.n_inputs)], param)
    # (reg.finish writes the fixed constant column: keygen's, not the witness's)
    if phased:
        return WitnessPlan._from_recorder(circuit, reg, params, [v.v.idx for v in outs], n_challenges=len(circuit.gc.cs.challenges),
                                          n_phases=1 + max(c.phase for c in circuit.gc.cs.advice))
    return WitnessPlan._from_recorder(circuit, reg, params, [v.v.idx for v in outs])


class WitnessPlan:
    def __init__(self, k, n_advice, n_inputs, params, consts, records, outputs, pool, n_cells, n_ops, param_hash, tables=(), table_values=(),
                 n_challenges=0, n_phases=1):
        """tables: (lo, n, col_size, offset into table_values) per static lookup table"""
        self.k, self.n_advice, self.n_inputs = k, n_advice, n_inputs
        self.n_challenges, self.n_phases = n_challenges, n_phases or 1
        self.tables = [tuple(int(v) for v in t) for t in tables]
        self.table_values = np.ascontiguousarray(table_values, np.int64).reshape(-1)
        self.params = np.ascontiguousarray(params, np.int64)
        self.consts = [int(c) for c in consts]
        self.records = np.ascontiguousarray(records, np.uint32).reshape(-1, 8)
        self.outputs = np.ascontiguousarray(outputs, np.uint32)
        self.pool = np.ascontiguousarray(pool, np.uint32)
        self.n_cells, self.n_ops, self.param_hash = n_cells, n_ops, bytes(param_hash)

    @classmethod
    def _from_recorder(cls, circuit, reg, params, outputs, n_challenges=0, n_phases=1):
        pool, records, n_cells = [], [], 0
        off = 0
        def push(a):
            nonlocal off
            a = np.asarray(a, np.uint32).reshape(-1)
            pool.append(a)
            off += len(a)
            return off - len(a)
        for rec in sorted(reg.out.recs, key=lambda r: r["phase"]):     # stable: a record reads cells of its own phase or an earlier one
            phase = rec["phase"]
            if rec["kind"] == RLC:
                src, dst = (np.array([sc[t] for sc in rec["scans"]], np.uint32).T for t in (0, 1))     # step-major
                n_cells += dst.size
                records.append([RLC, len(rec["scans"]), rec["p0"], rec["p1"], push(dst), push(src), 0, phase])
            elif rec["kind"] == MATMUL:
                if None in rec["dst"]:
                    raise PlanError("a matmul output is never placed")
                n_cells += len(rec["dst"])
                records.append([MATMUL, len(rec["dst"]), rec["p0"], rec["p1"], push(rec["dst"]), push(rec["a"]), push(rec["b"]), phase])
            elif rec["kind"] in (SUMACC, PRODACC):
                w, scans = rec["p0"], rec["scans"]
                nd, ns = len(scans), max(len(sc) for sc in scans)
                dst = np.full((ns, nd), NONE, np.uint32)
                a = np.full((ns, w, nd), NONE, np.uint32)
                for d, steps in enumerate(scans):
                    for s, (cell, cells) in enumerate(steps):
                        dst[s, d] = cell
                        a[s, :len(cells), d] = cells
                    n_cells += len(steps)
                records.append([rec["kind"], nd, w, ns, push(dst), push(a), 0, phase])
            elif rec["kind"] in (SORT, ARGSORT):
                src, dst = ([c for sc in rec["scans"] for c in sc[t]] for t in (0, 1))     # segment-major
                n_cells += len(dst)
                records.append([rec["kind"], len(dst), rec["p0"], rec["p1"], push(dst), push(src), 0, phase])
            elif rec["kind"] == ARGEXT:
                src, dst = [c for sc in rec["scans"] for c in sc[0]], [sc[1] for sc in rec["scans"]]     # segment-major
                n_cells += len(dst)
                records.append([ARGEXT, len(dst), rec["p0"], rec["p1"], push(dst), push(src), 0, phase])
            elif rec["kind"] == SCATTER:                   # b: the extent, the index cells, the source cells, the constant offsets
                job = rec["scans"][0]
                n_cells += len(job.dst)
                records.append([SCATTER, len(job.dst), len(job.index), job.mult, push(job.dst), push(job.base),
                                push([job.extent] + list(job.index) + list(job.src) + list(job.offsets)), phase])
            elif rec["kind"] == COMPLEMENT:
                job = rec["scans"][0]
                n_cells += len(job.dst)
                records.append([COMPLEMENT, len(job.dst), job.n, len(job.src), push(job.dst), push(job.src), 0, phase])
            elif rec["kind"] == RECIP:
                n_cells += len(rec["dst"])
                records.append([RECIP, len(rec["dst"]), rec["p0"], rec["p1"], push(rec["dst"]), push(rec["a"]), rec["scalar"], phase])
            elif rec["kind"] == GATHER:
                n = len(rec["dst"])
                n_cells += n
                records.append([GATHER, n, push(reg.gather_tables[rec["p0"]]), rec["p1"], push(rec["dst"]), push(rec["a"]), 0, phase])
            elif rec["kind"] == DOT:
                w, dots = rec["p0"], rec["dots"]
                nd, ns = len(dots), max(len(d) for d in dots)
                dst = np.full((ns, nd), NONE, np.uint32)
                a = np.full((ns, w, nd), NONE, np.uint32)
                b = np.full((ns, w, nd), NONE, np.uint32)
                for d, steps in enumerate(dots):
                    for s, (cell, pairs) in enumerate(steps):
                        dst[s, d] = cell
                        for j, (x, y) in enumerate(pairs):
                            a[s, j, d], b[s, j, d] = x, y
                    n_cells += len(steps)
                records.append([DOT, nd, w, ns, push(dst), push(a), push(b), phase])
            else:
                n = len(rec["dst"])
                n_cells += n
                records.append([rec["kind"], n, rec["p0"], rec["p1"], push(rec["dst"]), push(rec["a"]), push(rec["b"]) if rec["b"] else 0, phase])
        tables, values = [], []
        for lo, col_size, vals in getattr(reg, "tables", ()):
            tables.append((lo, len(vals), col_size, sum(len(v) for v in values)))
            values.append(vals)
        return cls(circuit.k, reg.n_adv, circuit.n_inputs, params, reg.consts, records, outputs,
                   np.concatenate(pool) if pool else np.zeros(0, np.uint32), n_cells, reg.n_ops, params_hash(circuit),
                   tables, np.concatenate(values) if values else (), n_challenges, n_phases)

    # ---- the blob ------------------------------------------------------------------------------------------------------------------------
    def to_bytes(self):
        head = _HEADER.pack(MAGIC, VERSION, self.k, self.n_advice, len(self.records), self.n_inputs, len(self.params), len(self.consts),
                            len(self.outputs), self.n_cells, len(self.pool), self.n_ops, len(self.tables), len(self.table_values), self.n_challenges,
                            self.n_phases if self.n_phases > 1 else 0, 0, 0, 0, 0, self.param_hash)
        directory = b"".join(struct.pack("<iIII", *t) for t in self.tables)
        return b"".join([head, self.params.astype("<i8").tobytes(), b"".join(c.to_bytes(32, "little") for c in self.consts),
                         self.records.astype("<u4").tobytes(), self.outputs.astype("<u4").tobytes(), self.pool.astype("<u4").tobytes(),
                         directory, self.table_values.astype("<i8").tobytes()])

    @classmethod
    def from_bytes(cls, blob):
        blob = bytes(blob)
        if len(blob) < _HEADER.size:
            raise PlanError("witness plan: shorter than its header")
        f = _HEADER.unpack_from(blob)
        if f[0] != MAGIC:
            raise PlanError("witness plan: bad magic")
        if f[1] != VERSION:
            raise PlanError("witness plan: version %d, this build reads %d" % (f[1], VERSION))
        _, _, k, n_adv, n_rec, n_in, n_par, n_con, n_out, n_cells, n_words, n_ops, n_tab, n_val = f[:14]
        sizes = [8 * n_par, 32 * n_con, 32 * n_rec, 4 * n_out, 4 * n_words, 16 * n_tab, 8 * n_val]
        if len(blob) != _HEADER.size + sum(sizes):
            raise PlanError("witness plan: %d bytes, its header says %d" % (len(blob), _HEADER.size + sum(sizes)))
        o = [_HEADER.size]
        for s in sizes:
            o.append(o[-1] + s)
        params = np.frombuffer(blob, "<i8", n_par, o[0])
        consts = [int.from_bytes(blob[o[1] + 32 * i:o[1] + 32 * i + 32], "little") for i in range(n_con)]
        records = np.frombuffer(blob, "<u4", 8 * n_rec, o[2])
        outputs = np.frombuffer(blob, "<u4", n_out, o[3])
        pool = np.frombuffer(blob, "<u4", n_words, o[4])
        tables = [struct.unpack_from("<iIII", blob, o[5] + 16 * i) for i in range(n_tab)]
        values = np.frombuffer(blob[o[6]:o[7]], "<i8")
        return cls(k, n_adv, n_in, params, consts, records, outputs, pool, n_cells, n_ops, f[20], tables, values, f[14], f[15])

    def __eq__(self, other):
        return isinstance(other, WitnessPlan) and self.to_bytes() == other.to_bytes()

    @property
    def n_records(self):
        return len(self.records)

    def validate(self):
        validate(self)
        return self


def peek(blob):
    """the header of a plan blob: what `prove` compares with the compiled circuit before it uploads the blob"""
    if len(blob) < _HEADER.size:
        raise PlanError("witness plan: shorter than its header")
    f = _HEADER.unpack_from(blob)
    if f[0] != MAGIC or f[1] != VERSION:
        raise PlanError("witness plan: bad magic or version")
    names = ["k", "n_advice", "n_records", "n_inputs", "n_params", "n_consts", "n_outputs", "n_cells", "n_words", "n_ops", "n_tables", "n_table_values"]
    return dict(zip(names, f[2:14]), n_challenges=f[14], n_phases=f[15] or 1, param_hash=f[20])


def _i32(w):
    return w - (1 << 32) if w >> 31 else w


def _span(plan, off, n, what, ri):
    if off > len(plan.pool) or n > len(plan.pool) - off:
        raise PlanError("witness plan: record %d: %s runs past the pool" % (ri, what))
    return plan.pool[off:off + n]


class _Written:
    """the set of cells written so far, as csrc/witness_plan.hpp keeps it: memory bounded by the blob, not by the geometry its header claims
    -- one flag per cell when that is no more than the pool itself, otherwise one per distinct pool word (binary search)"""

    def __init__(self, cells, pool):
        self.keys = None if cells <= 32 * len(pool) + (1 << 19) else np.unique(pool)
        self.flags = np.zeros(cells if self.keys is None else len(self.keys), bool)

    def _at(self, x):
        if self.keys is None:
            return x, np.ones(len(x), bool)
        i = np.minimum(np.searchsorted(self.keys, x), max(len(self.keys) - 1, 0))
        return i, (self.keys[i] == x if len(self.keys) else np.zeros(len(x), bool))

    def get(self, x):
        i, known = self._at(x)
        return self.flags[i] & known if len(self.flags) else known

    def set(self, x):
        self.flags[self._at(x)[0]] = True


def _refuse(ri, kind, words):
    """a record refused; kind None: the messages that do not name the kind"""
    return PlanError("witness plan: record %d%s: %s" % (ri, "" if kind is None else " (%s)" % KIND_NAMES[kind], words))


def validate(plan):
    """the check ezkl_hip_witness_plan_upload makes before anything reaches the device, mirrored: geometry, every cell index below
    n_advice * 2^k, every table index in range, every lookup table inside the table values, every cell written at most once and read only
    after an EARLIER record wrote it, the phases non-decreasing and below n_phases, every column written in one phase only.  A kind's case
    checks its own parameters and says which words it has; what holds for every kind is checked once, after the cases"""
    if not 1 <= plan.k <= 28 or not 0 < plan.n_advice <= 64 or (plan.n_advice << plan.k) > 1 << 32:
        raise PlanError("witness plan: bad geometry")
    cells = plan.n_advice << plan.k
    if not 1 <= plan.n_phases <= MAX_PHASES or plan.n_challenges > MAX_CHALLENGES:
        raise PlanError("witness plan: bad phase or challenge count")
    if any(c >= R for c in plan.consts):
        raise PlanError("witness plan: a constant is not a canonical field element")
    if plan.n_cells > len(plan.pool):
        raise PlanError("witness plan: more cells than index words")
    for ti, (lo, n, col_size, off) in enumerate(plan.tables):
        if n < 1 or col_size < 1 or lo + n - 1 > (1 << 31) - 1:
            raise PlanError("witness plan: table %d: bad lookup table shape" % ti)
        if off > len(plan.table_values) or n > len(plan.table_values) - off:
            raise PlanError("witness plan: table %d: runs past the table values" % ti)
    written = _Written(cells, plan.pool)
    total, words = 0, len(plan.pool)
    fits = lambda off, n: off <= words and n <= words - off
    col_phase, last_phase = [None] * plan.n_advice, 0
    for ri, (kind, count, p0, p1, dst, a, b, phase) in enumerate(plan.records.tolist()):
        if kind >= KINDS_TOP or kind in UNASSIGNED_KINDS:
            raise PlanError("witness plan: record %d: unknown kind %d" % (ri, kind))
        if count == 0 and kind != COMPLEMENT:             # (nothing missing: a complement that writes no cell)
            raise PlanError("witness plan: record %d is empty" % ri)
        if phase >= plan.n_phases:
            raise _refuse(ri, kind, "phase out of range")
        if phase < last_phase:
            raise _refuse(ri, kind, "phases decrease")
        last_phase = phase
        if kind in (INPUT, MATMUL) and phase != 0:
            raise _refuse(ri, kind, "input and matmul records belong to phase 0")
        # the kind's own parameters, and the words it has: n_dst at dst, n_a at a, n_b at b, lim for its indices, `extra` further cells a lane reads
        K, n_dst = KINDS[kind], dst_words(kind, count, p1)
        n_a, n_b, lim, extra = count, 0, 0, None
        if kind in (ADD, SUB, MUL, ONEHOT):               # (ONEHOT: the position each element stands for, plain words)
            n_b = count
            if kind == ONEHOT and p0 == 0:
                raise _refuse(ri, kind, "zero one-hot classes")
        elif kind in (CONST, INPUT, PARAM):
            lim = {CONST: len(plan.consts), INPUT: plan.n_inputs, PARAM: len(plan.params)}[kind]
        elif kind == HINT:                                # p0 = base, p1 = legs; b: the digit of each element, below p1
            n_b, lim = count, p1
            if p0 < 2 or p1 == 0 or p0 ** p1 >= 1 << 62:
                raise _refuse(ri, None, "bad decomposition")
        elif kind == RCIDX and p1 == 0:
            raise _refuse(ri, None, "zero table column size")
        elif kind == DIVC and p0 == 0:
            raise _refuse(ri, None, "zero divisor")
        elif kind in (TABLE, TBLIDX) and p0 >= len(plan.tables):
            raise _refuse(ri, kind, "lookup table index out of range")
        elif kind == MATMUL:                              # p0 = kd, p1 = n, count = m * n: a = m * kd, b = kd * n input indices
            if p0 == 0 or p1 == 0 or count % p1 != 0 or not (fits(dst, count) and fits(a, count // p1 * p0) and fits(b, p0 * p1)):
                raise _refuse(ri, kind, "bad matmul shape")
            n_a, n_b, lim = count // p1 * p0, p0 * p1, plan.n_inputs
        elif kind == RLC:                                 # p0 = challenge, p1 = steps, count = scans
            if p0 >= plan.n_challenges:
                raise _refuse(ri, kind, "challenge index out of range")
            if p1 == 0 or n_dst > words:
                raise _refuse(ri, kind, "bad rlc shape")
            n_a = n_dst
        elif kind in (SUMACC, PRODACC):                   # p0 = operands per step, p1 = steps, count = scans
            n_a = n_dst * p0
            if p0 == 0 or p1 == 0 or not (fits(dst, n_dst) and fits(a, n_a)):
                raise _refuse(ri, kind, "bad scan shape")
        elif kind == GATHER:                              # p0 = pool offset of the table's cell list, p1 = its length: cells a lane reads
            if p1 == 0:
                raise _refuse(ri, kind, "empty gather table")
            if not fits(p0, p1):
                raise _refuse(ri, kind, "gather table runs past the pool")
            extra = plan.pool[p0:p0 + p1]
        elif kind == CLAMP and _i32(p0) > _i32(p1):
            raise _refuse(ri, kind, "bad clamp bounds")
        elif kind in (SORT, ARGSORT):                     # p0 = segment length, p1 = mode, count = segments * p0
            if p0 == 0 or count % p0 != 0 or p1 > 1 or count > MAX_SORT_COUNT:
                raise _refuse(ri, kind, "bad sort shape")
        elif kind == RECIP:                               # S = p0 | p1 << 32; b: the constant a zero input takes
            if not 1 <= (p0 | p1 << 32) < 1 << 62:
                raise _refuse(ri, kind, "reciprocal scale outside [1, 2^62)")
            if b >= len(plan.consts):
                raise _refuse(ri, kind, "zero-inverse index past the constants")
        elif kind == ISQRT:
            if p0 == 0:
                raise _refuse(ri, kind, "zero square-root scale")
            if p1 != 0:
                raise _refuse(ri, kind, "a square-root record with a second parameter")
        elif kind == ARGEXT:                              # p0 = segment length, p1 = mode, count = segments = destination cells
            n_a = count * p0
            if p0 == 0 or p1 > 1 or n_a > MAX_SORT_COUNT or not (fits(dst, count) and fits(a, n_a)):
                raise _refuse(ri, kind, "bad arg-extremum shape")
        elif kind == SCATTER:                             # p0 = elements, p1 = multiplier, b: extent, index cells, source cells, offsets
            n_b = 1 + 3 * p0
            ok = p0 >= 1 and p1 >= 1 and count <= MAX_SORT_COUNT and fits(dst, count) and fits(a, count) and fits(b, n_b)
            if ok:
                extent = int(plan.pool[b])
                ok = extent >= 1 and int(plan.pool[b + 1 + 2 * p0:b + 1 + 3 * p0].max()) + (extent - 1) * p1 < count
            if not ok:
                raise _refuse(ri, kind, "bad scatter shape")
            extra = plan.pool[b + 1:b + 1 + 2 * p0]       # the index and source cells: ones a lane reads
        elif kind == COMPLEMENT:                          # p0 = n, p1 = sources, count = n - sources
            n_a = p1
            if p1 > p0 or count != p0 - p1 or p0 > MAX_SORT_COUNT or not (fits(dst, count) and fits(a, p1)):
                raise _refuse(ri, kind, "bad complement shape")
        elif kind == DOT:                                 # p0 = products per step, p1 = steps, count = dot products
            n_a = n_b = n_dst * p0
            if p0 == 0 or p1 == 0 or n_a > words:
                raise _refuse(ri, None, "bad dot shape")
        # what holds for every kind
        d, xa = _span(plan, dst, n_dst, "dst", ri), _span(plan, a, n_a, "a", ri)
        xb = _span(plan, b, n_b, "b", ri) if n_b else xa[:0]
        if K.sparse and n_b and ((xa == NONE) != (xb == NONE)).any():
            raise _refuse(ri, kind, "a product with one operand")
        for role, x in ((K.a, xa), (K.b, xb)):
            if role == INDICES and (x >= lim).any():
                raise _refuse(ri, kind, "table index out of range")
            if role == DIGITS and ((x != NONE) & (x >= lim)).any():
                raise _refuse(ri, None, "bad decomposition")
        srcs = [x for role, x in ((K.a, xa), (K.b, xb)) if role == CELLS] + ([extra] if extra is not None else [])
        srcs = srcs[0] if len(srcs) == 1 else np.concatenate(srcs) if srcs else xa[:0]
        if K.sparse:                                      # 0xffffffff: no entry
            srcs, d = srcs[srcs != NONE], d[d != NONE]
        if (d >= cells).any() or (srcs >= cells).any():
            raise _refuse(ri, kind, "cell index out of range")
        if not written.get(srcs).all():
            raise _refuse(ri, kind, "a cell is read before an earlier record has written it")
        if written.get(d).any() or len(np.unique(d)) != len(d):
            raise _refuse(ri, kind, "a cell is written twice")
        written.set(d)
        total += len(d)
        for c in np.unique(d >> plan.k).tolist():
            if col_phase[c] is not None and col_phase[c] != phase:
                raise _refuse(ri, kind, "a column is written in two phases")
            col_phase[c] = phase
    if total != plan.n_cells:
        raise PlanError("witness plan: %d cells written, its header says %d" % (total, plan.n_cells))
    if (plan.outputs >= cells).any() or not written.get(plan.outputs).all():
        raise PlanError("witness plan: an output cell is never written")


def _written_cells(plan, kind, count, p1, dst):
    d = plan.pool[dst:dst + dst_words(kind, count, p1)]
    return d[d != NONE] >> plan.k


def column_phases(plan):
    """the phase each advice column belongs to: that of the records that write it (`validate` refuses two), 0 for a column no record writes"""
    out = [0] * plan.n_advice
    for kind, count, p0, p1, dst, a, b, phase in plan.records.tolist():
        for c in np.unique(_written_cells(plan, kind, count, p1, dst)).tolist():
            out[c] = phase
    return out


def written_columns(plan):
    """the advice columns some record writes a cell of (every other column is all zeros after its phase has run)"""
    out = set()
    for kind, count, p0, p1, dst, a, b, phase in plan.records.tolist():
        out.update(_written_cells(plan, kind, count, p1, dst).tolist())
    return out


STATS_ERROR = "lookup input beyond 62 bits"


def lookup_stats_host(plan, columns):
    """(min_lookup_inputs, max_lookup_inputs) of a replayed plan, in Python integers: the executable specification of
    ezkl_hip_witness_lookup_stats_dev.  Over every TABLE record, in all phases, the least and the greatest signed value of the source
    cells pool[a + i], both folded with 0 -- what BaseRegion.nonlinearity keeps as it lays the same circuit out.  columns: the advice
    columns as canonical integers (run_plan_host's).  A source whose magnitude needs 62 bits or more is refused (ValueError), never
    folded in: no column of a replay that passed holds one there."""
    n = 1 << plan.k
    lo = hi = 0
    P = plan.pool.tolist()
    for kind, count, p0, p1, dst, a, b, phase in plan.records.tolist():
        if kind != TABLE:
            continue
        for i in range(count):
            c = P[a + i]
            s = EL.signed(int(columns[c >> plan.k][c & (n - 1)]) % R)
            if abs(s) >= 1 << 62:
                raise ValueError(STATS_ERROR)
            lo, hi = min(lo, s), max(hi, s)
    return lo, hi


def _lane_failure(kind, ri, element):
    """the run-time failure of a lane, worded as the device words it (csrc/witness.hip)"""
    return AssertionError("%s (%s record %d, element %d)" % (KINDS[kind].failure, KIND_NAMES[kind], ri, element))


def run_plan_host(plan, x, challenges=None, phase=None):
    """interpret the plan with Python integers -> (advice columns as lists of canonical ints, outputs).  Record by record, element by
    element, what one lane of the device kernels does.  A plan with phases: with `challenges` (canonical ints) every phase is
    interpreted; phase=0 interprets the first phase alone (the later columns stay zero, and so do the outputs)."""
    validate(plan)
    if len(x) != plan.n_inputs:
        raise ValueError("the plan takes %d inputs, got %d" % (plan.n_inputs, len(x)))
    if phase not in (None, 0):
        raise ValueError("the host interpreter runs every phase, or phase 0 alone")
    challenges = [int(c) % R for c in challenges] if challenges is not None else []
    if phase is None and plan.n_phases > 1 and len(challenges) < plan.n_challenges:
        raise ValueError("the plan takes %d challenges, got %d" % (plan.n_challenges, len(challenges)))
    n = 1 << plan.k
    cells = [0] * (plan.n_advice * n)
    P, params, consts = plan.pool.tolist(), plan.params.tolist(), plan.consts
    xs = [int(v) for v in x]
    for ri, (kind, count, p0, p1, dst, a, b, rec_phase) in enumerate(plan.records.tolist()):
        if phase is not None and rec_phase > phase:
            break
        if kind == MATMUL:
            kd, nn = p0, p1
            m = count // nn
            ia, ib = P[a:a + m * kd], P[b:b + kd * nn]
            for e, i in enumerate(ia + ib):                # every operand a lane reads, the smallest failing element first
                if abs(xs[i]) >= 1 << 31:
                    raise _lane_failure(kind, ri, e)
            for i in range(m):
                for j in range(nn):
                    cells[P[dst + i * nn + j]] = sum(xs[ia[i * kd + t]] * xs[ib[t * nn + j]] for t in range(kd)) % R
            continue
        if kind == RLC:
            c = challenges[p0]
            for d in range(count):
                acc = 0
                for t in range(p1):
                    acc = (acc * c + c * cells[P[a + t * count + d]]) % R
                    cells[P[dst + t * count + d]] = acc
            continue
        if kind == DOT:
            w, ns = p0, p1
            for d in range(count):
                acc = 0
                for s in range(ns):
                    cell = P[dst + s * count + d]
                    if cell == NONE:
                        continue
                    for j in range(w):
                        ia = P[a + (s * w + j) * count + d]
                        if ia != NONE:
                            acc = (acc + cells[ia] * cells[P[b + (s * w + j) * count + d]]) % R
                    cells[cell] = acc
            continue
        if kind in (SUMACC, PRODACC):
            w, ns = p0, p1
            for d in range(count):
                acc = 0 if kind == SUMACC else 1
                for s in range(ns):
                    cell = P[dst + s * count + d]
                    if cell == NONE:
                        continue
                    for j in range(w):
                        ia = P[a + (s * w + j) * count + d]
                        if ia != NONE:
                            acc = (acc + cells[ia]) % R if kind == SUMACC else acc * cells[ia] % R
                    cells[cell] = acc
            continue
        if kind == ARGEXT:
            vals = [EL.signed(cells[c]) for c in P[a:a + count * p0]]
            for e, sv in enumerate(vals):                  # every source a lane reads, the smallest failing element first
                if abs(sv) >= 1 << 62:
                    raise _lane_failure(kind, ri, e)
            for g in range(count):
                seg = vals[g * p0:(g + 1) * p0]
                cells[P[dst + g]] = seg.index(min(seg) if p1 else max(seg))     # the first position that holds the extremum
            continue
        if kind == SCATTER:                                # the greatest element on a target wins: the elements in order, each overwriting
            extent, m = P[b], p0
            idx = [EL.signed(cells[c]) for c in P[b + 1:b + 1 + m]]
            for j, sv in enumerate(idx):                   # every index a lane reads, the smallest failing element first
                if sv < 0 or sv >= extent or abs(sv) >= 1 << 62:
                    raise _lane_failure(kind, ri, j)
            out = [cells[c] for c in P[a:a + count]]
            for j, sv in enumerate(idx):
                out[sv * p1 + P[b + 1 + 2 * m + j]] = cells[P[b + 1 + m + j]]
            for i, v in enumerate(out):
                cells[P[dst + i]] = v
            continue
        if kind == COMPLEMENT:                             # the positions no source names, ascending, as many as the record has cells
            named = {EL.signed(cells[c]) for c in P[a:a + p1]}
            rest = [v for v in range(p0) if v not in named]
            for i in range(count):
                cells[P[dst + i]] = rest[i]
            continue
        if kind in (SORT, ARGSORT):
            vals = [EL.signed(cells[c]) for c in P[a:a + count]]
            for e, sv in enumerate(vals):                  # every source a lane reads, the smallest failing element first
                if abs(sv) >= 1 << 62:
                    raise _lane_failure(kind, ri, e)
            for g in range(0, count, p0):
                seg = vals[g:g + p0]
                for i, j in enumerate(sorted(range(p0), key=lambda j: (seg[j], -j if p1 else j))):
                    cells[P[dst + g + i]] = seg[j] % R if kind == SORT else j
            continue
        lo = p0 - (1 << 32) if p0 >> 31 else p0
        for i in range(count):
            ia = P[a + i]
            if kind == COPY: v = cells[ia]
            elif kind == CONST: v = consts[ia]
            elif kind == INPUT: v = xs[ia] % R
            elif kind == PARAM: v = params[ia] % R
            elif kind == ADD: v = (cells[ia] + cells[P[b + i]]) % R
            elif kind == SUB: v = (cells[ia] - cells[P[b + i]]) % R
            elif kind == MUL: v = cells[ia] * cells[P[b + i]] % R
            elif kind == INVZ: v = pow(cells[ia], -1, R) if cells[ia] else 0
            elif kind in (TABLE, TBLIDX):
                t_lo, t_n, t_col, t_off = plan.tables[p0]
                s = EL.signed(cells[ia])
                if s < t_lo or s > t_lo + t_n - 1 or abs(s) >= 1 << 62:
                    raise _lane_failure(kind, ri, i)
                v = int(plan.table_values[t_off + s - t_lo]) % R if kind == TABLE else (s - t_lo) // t_col
            elif kind == DIVC:
                s = EL.signed(cells[ia])
                if abs(s) >= 1 << 52:
                    raise _lane_failure(kind, ri, i)
                v = EL.round_div(s, p0) % R
            elif kind == GATHER:                          # the index is tested before it is used
                s = EL.signed(cells[ia])
                if s < 0 or s >= p1 or abs(s) >= 1 << 62:
                    raise _lane_failure(kind, ri, i)
                v = cells[P[p0 + s]]
            elif kind == CLAMP:                           # beyond 62 bits: by its sign, as the lane does
                v = min(max(EL.signed(cells[ia]), lo), _i32(p1)) % R
            elif kind == RECIP:                           # the claim rule is the layout's, in exact integers
                s = EL.signed(cells[ia])
                if abs(s) >= 1 << 62:
                    raise _lane_failure(kind, ri, i)
                v = consts[b] if s == 0 else EL.recip_claim(s, p0 | p1 << 32, 0) % R
            elif kind == ISQRT:
                s = EL.signed(cells[ia])
                if abs(s) >= 1 << 62 or s * p0 >= 1 << 62:
                    raise _lane_failure(kind, ri, i)
                v = EL.sqrt_claim(s, p0)
            elif kind == ONEHOT:
                s = EL.signed(cells[ia])
                if s < 0 or s >= p0 or abs(s) >= 1 << 62:
                    raise _lane_failure(kind, ri, i)
                v = int(s == P[b + i])
            elif kind == RCIDX:
                s = EL.signed(cells[ia])
                if abs(s) >= 1 << 62:                 # what a lane holds in 64 bits; the layout only range-checks signs and digits
                    raise _lane_failure(kind, ri, i)
                v = abs(s - lo) // p1
            else:
                s, e = EL.signed(cells[ia]), P[b + i]
                if abs(s) >= p0 ** p1:
                    raise _lane_failure(kind, ri, i)
                v = ((s > 0) - (s < 0)) % R if e == NONE else (abs(s) // p0 ** e) % p0
            cells[P[dst + i]] = v
    done = phase is None or phase == plan.n_phases - 1
    return [cells[c * n:(c + 1) * n] for c in range(plan.n_advice)], [cells[c] for c in plan.outputs.tolist()] if done else []
