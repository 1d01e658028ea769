"""Quotient-sweep programs that OVERWRITE their intermediates, shared by tests/test_evalh_forms_cpu.py (scheduler, slot check, generated
source and oracle against a big-int evaluation, CPU) and tests/test_gpu_evalh_forms.py (the four kernels, GPU).

Every other program of the suite comes out of GraphProgram.calc with a fresh intermediate index per instruction.  The library promises
more (include/ezkl_hip.h): an index may be rewritten any number of times, a Horner step on a never-written target is its term, a read of
a never-written intermediate is refused, and the result is the last instruction's target.  The forms below are built on those rules:
schedule_program's write-after-read and write-after-write edges, allocate_slots' release and re-acquire of a slot across the versions
of one index, the version tables of the three code generators and "the check follows the LAST write" of the check kernel all only show
on programs like these.

Operands cycle over every (column, rotation -2..2), the challenges, the edge constants of evalh_programs.CONST_WORDS and `previous`
(Builder.load; tests/test_evalh_forms_cpu.py asserts the coverage); every program has a fixed seed and stays below ~150 instructions (hiprtc time per program well under a second)."""
import numpy as np

import evalh_programs as EP

N_COLUMNS = EP.N_COLUMNS
N_CHALLENGES = EP.N_CHALLENGES
K, EXT_K = EP.K, EP.EXT_K
P = EP.R
CONST, INTERMEDIATE, COLUMN, CHALLENGE, PREVIOUS = range(5)
HORNER = 7
UNARY = (3, 4, 5, 6)                 # square, double, negate, store


# ---- words ------------------------------------------------------------------------------------------------------------------------
def _words(ints):
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in ints), np.uint64).reshape(-1, 4).copy()


def _ints(a):
    b = np.ascontiguousarray(a, np.uint64).tobytes()
    return [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(len(b) // 32)]


def _draw(rng, n):
    """n words, each drawn from: p - 1, 0, 1, p - 2, (p -+ 1) / 2, uniform over [2^253, p), uniform over all of [0, p)"""
    special = [P - 1, 0, 1, P - 2, (P - 1) // 2, (P + 1) // 2]
    kind = rng.integers(0, 8, n)
    out = []
    for i in range(n):
        k = int(kind[i])
        if k < 6:
            out.append(special[k])
        else:
            lo = (1 << 253) if k == 6 else 0
            w = int.from_bytes(rng.bytes(32), "little") % (P - lo) + lo      # bias < 2^-250
            out.append(w)
    return out


# ---- the builder ------------------------------------------------------------------------------------------------------------------
class Builder(EP.Builder):
    """evalh_programs.Builder with a load cycle of its own -- five columns, a challenge, a constant, `previous`, over and over; the
    columns walk all 4 x 5 (column, rotation) pairs, the constants all of CONST_WORDS -- and a calc that takes its target"""

    def __init__(self, B, k=K, ext_k=EXT_K):
        super().__init__(B, k, ext_k)
        self.n_col = self.n_chal = self.n_const = 0

    def load(self):
        m = self.i % 8
        self.i += 1
        if m == 7:
            return self.p.previous()
        if m == 6:
            self.n_const += 1
            return self.p.constant(EP.word(EP.CONST_WORDS[(self.n_const - 1) % len(EP.CONST_WORDS)]))
        if m == 5:
            self.n_chal += 1
            return self.p.challenge((self.n_chal - 1) % N_CHALLENGES)
        self.n_col += 1
        return self.p.column((self.n_col - 1) % N_COLUMNS, (self.n_col - 1) % 5 - 2)

    def new(self):
        """an intermediate index of its own, not yet written"""
        t = self.p.n_intermediates
        self.p.n_intermediates += 1
        return t

    def put(self, t, name, a, b=None):
        """instruction `name` with target t -> the source that reads t"""
        return self.p.calc(name, a, target=t) if b is None else self.p.calc(name, a, b, target=t)


def I(t):
    return (INTERMEDIATE, t, 0)


# ---- ring_R: a random DAG whose targets come from a ring of R indices ----------------------------------------------------------------
def ring(B, R, seed, n=110, k=K, ext_k=EXT_K, fresh_horner=()):
    """every target is one of R indices, so each is overwritten many times (R = 3: inside the interpreter's 8 registers; 8 and 9: on both
    sides of them by index count; 10: one spilled slot; 40: many, see RINGS).  An intermediate source is an index written at that point.  Every third instruction is planted
    right behind its predecessor as a pure hazard: it overwrites an index the predecessor read (write after read), or the predecessor's
    own target without reading it (write after write).  The tail is halo2's: one Horner chain over the last values"""
    rng = np.random.default_rng(seed)
    b = Builder(B, k, ext_k)
    p = b.p
    p.n_intermediates = R
    written = []                                       # indices written so far, most recent last
    ops2, ops1 = ["add", "sub", "mul"], ["square", "double", "negate", "store"]
    zero = p.constant(EP.word(0))

    def src(avoid=(), chain=False):
        live = [x for x in written if x not in avoid]
        if chain and live and rng.random() < 0.6:      # operand 0 is an intermediate, mostly the value just written: much of the
            return I(live[-1])                         # program then reaches the result
        if live and (chain or rng.random() < 0.6):
            j = live[-1 - int(rng.integers(0, min(len(live), 5)))] if rng.random() < 0.7 else live[int(rng.integers(0, len(live)))]
            return I(j)
        return b.load()

    for it in range(n):
        if it in fresh_horner:                         # a Horner step on a never-written index (its term) while many values are live
            t = b.new()
            b.put(t, "horner_step", src(chain=True), b.load())
            written.append(t)
        plant = it % 6
        prev_ins = p.code[-1] if p.code else None
        avoid = ()
        t = int(rng.integers(0, R))
        if prev_ins is not None and plant == 5:       # write after write: the predecessor's target again, neither reading the other
            t = prev_ins[1]
            avoid = (t,)
        elif prev_ins is not None and plant == 2:     # write after read: an index the predecessor read, not reading its result
            reads = [prev_ins[3 + 3 * q] for q in range(1 if prev_ins[0] in UNARY else 2) if prev_ins[2 + 3 * q] == INTERMEDIATE]
            reads = [x for x in reads if x != prev_ins[1]]
            if reads:
                t = reads[0]
                avoid = (prev_ins[1],)
        if rng.random() < 0.75:
            name = ops2[int(rng.integers(0, 3))]
            s0, s1 = src(avoid, chain=True), src(avoid)
            if name == "sub" and s0 == s1:             # x - x: a zero that would swallow every product it meets
                s1 = b.load()
            if name == "mul" and zero in (s0, s1):     # and so would the constant 0: it is added instead
                name = "add"
            if rng.random() < 0.5:                     # loads in both operand positions
                s0, s1 = s1, s0
            b.put(t, name, s0, s1)
        else:
            b.put(t, ops1[int(rng.integers(0, 4))], src(avoid, chain=True))
        if t in written:
            written.remove(t)
        written.append(t)
    p.horner(p.previous(), [I(x) for x in written[-12:]], p.challenge(0))
    return p


# ---- self_update: non-Horner instructions whose target is one of their own sources -----------------------------------------------------
def self_update(B, k=K, ext_k=EXT_K):
    """t = t + x, t = x - t, t = t * t (mul and square), double, negate and store t <- t, each index in both operand positions, three rounds:
    the adds and doublings push alpha and L of the radix-2^29 generator up version after version, so every version needs its own state.
    Two running values read each other (write-after-read pairs), and t starts with a write nobody reads (a write-after-write pair)"""
    b = Builder(B, k, ext_k)
    t, u = b.new(), b.new()
    b.put(t, "store", b.load())                        # dead: overwritten by the next instruction
    b.put(t, "add", b.load(), b.load())
    b.put(u, "mul", b.load(), b.load())
    for _ in range(3):
        b.put(t, "add", I(t), b.load())                # t = t + x
        b.put(u, "add", b.load(), I(u))                # u = x + u
        b.put(t, "sub", b.load(), I(t))                # t = x - t
        b.put(u, "sub", I(u), b.load())                # u = u - x
        b.put(t, "add", I(t), I(u))                    # reads u ...
        b.put(u, "square", I(u))                       # ... which the next instruction overwrites without reading t
        b.put(t, "mul", I(t), I(t))                    # t = t * t as a product
        b.put(u, "mul", b.load(), I(u))                # u = x * u
        b.put(t, "mul", I(t), b.load())                # t = t * x
        b.put(t, "double", I(t))
        b.put(t, "double", I(t))
        b.put(u, "negate", I(u))
        b.put(t, "store", I(t))                        # store t <- t
        b.put(u, "sub", I(t), I(u))                    # u = t - u
        b.put(t, "add", I(t), I(t))                    # both operands
    b.put(t, "add", I(u), I(t))
    return b.p


def operand_sweep(B, k=K, ext_k=EXT_K):
    """one running value updated in place with every operand there is -- each (column, rotation -2 .. 2), each challenge, each
    CONST_WORDS entry and `previous` -- once as operand 0 and once as operand 1; the ops rotate over sub, mul and add (the constant 0 is
    added: a product with it would end the chain)"""
    b = Builder(B, k, ext_k)
    p = b.p
    xs = [p.column(c, r) for r in range(-2, 3) for c in range(N_COLUMNS)] + [p.challenge(c) for c in range(N_CHALLENGES)]
    xs += [p.constant(EP.word(w)) for w in EP.CONST_WORDS] + [p.previous()]
    t = b.new()
    b.put(t, "add", p.previous(), p.column(0, 0))
    for i, x in enumerate(xs):
        first, second = ("sub", "mul", "add")[i % 3], ("mul", "add", "sub")[i % 3]
        if x == p.constant(EP.word(0)):
            first, second = "add", "sub"
        b.put(t, first, x, I(t))
        b.put(t, second, I(t), x)
    return p


# ---- horner_forms ---------------------------------------------------------------------------------------------------------------------
def horner_mixed(B, k=K, ext_k=EXT_K):
    b = Builder(B, k, ext_k)
    f = b.op("add", b.load(), b.op("mul", b.load(), b.load()))        # the factor is an intermediate
    a = b.put(b.new(), "store", b.load())
    for _ in range(3):
        b.put(a[1], "horner_step", b.op("mul", b.load(), b.load()), f)
    b.put(a[1], "horner_step", a, b.load())                             # the term is the chain's own target: a = a * x + a
    b.put(a[1], "horner_step", b.load(), a)                             # the factor is the chain's own target: a = a * a + x
    b.put(a[1], "horner_step", a, a)                                    # both
    c, d = b.put(b.new(), "store", b.load()), b.put(b.new(), "store", b.load())
    for _ in range(3):                                                  # two interleaved chains, each reading the other's running value
        b.put(c[1], "horner_step", d, b.load())
        b.put(d[1], "horner_step", b.load(), c)
    e = b.put(b.new(), "store", b.load())                               # a chain interrupted by a store into its target, then resumed
    b.put(e[1], "horner_step", b.load(), f)
    b.put(e[1], "horner_step", c, f)
    b.put(e[1], "store", b.op("add", e, d))
    b.put(e[1], "horner_step", b.load(), f)
    b.put(e[1], "horner_step", a, b.load())
    g = b.op("mul", b.load(), b.load())                                 # an ordinary value ...
    h = b.op("add", g, e)
    b.put(g[1], "horner_step", h, f)                                    # ... then a step on its index: written, so the step is in place
    b.put(g[1], "horner_step", b.load(), b.load())
    return b.done(b.op("add", g, h))


def horner_first(B, factor, k=K, ext_k=EXT_K):
    """the first instruction is a Horner step on a never-written index: 0 * factor + term"""
    b = Builder(B, k, ext_k)
    fac = {"column": b.p.column(1, -1), "challenge": b.p.challenge(1), "previous": b.p.previous()}[factor]
    t = b.new()
    b.put(t, "horner_step", b.load(), fac)
    b.put(t, "horner_step", b.load(), fac)
    return b.done(b.op("add", I(t), b.load()))


# ---- dead_code ------------------------------------------------------------------------------------------------------------------------
def dead_code(B, k=K, ext_k=EXT_K):
    b = Builder(B, k, ext_k)
    res, x = b.new(), b.new()
    a = b.op("mul", b.load(), b.load())
    b.op("add", b.load(), b.load())                                     # a result nobody reads
    b.put(x, "sub", b.load(), b.load())                                 # a dead write: x is overwritten before anyone reads it
    b.op("square", a)                                                   # dead, but a reader of a
    b.put(res, "store", b.load())                                       # the result index, written early and never read as this
    b.put(x, "mul", a, b.load())
    y = b.op("add", I(x), b.load())
    z = b.p.horner(b.p.previous(), [y, a, I(x)], b.p.challenge(0))
    b.op("negate", z)                                                   # dead, behind the chain
    b.put(x, "double", y)                                               # dead last version of x
    b.put(res, "add", z, y)
    return b.p


def dead_horner(B, k=K, ext_k=EXT_K):
    """Horner steps are present (the scheduler starts from them) but the result does not depend on any"""
    b = Builder(B, k, ext_k)
    a = b.op("add", b.load(), b.load())
    b.p.horner(b.p.previous(), [a, b.load(), b.op("mul", a, b.load())], b.p.challenge(2))
    b.put(b.new(), "horner_step", a, b.load())                          # and one on a never-written index
    return b.done(b.op("mul", b.op("sub", a, b.load()), b.load()))


# ---- tiny -----------------------------------------------------------------------------------------------------------------------------
def tiny(B, k=K, ext_k=EXT_K):
    out = []
    for name in ("add", "sub", "mul", "square", "double", "negate", "store", "horner_step"):
        b = Builder(B, k, ext_k)
        p = b.p
        if name in ("square", "double", "negate", "store"):
            p.calc(name, p.column(2, 1))
        else:                                                           # the lone Horner step is on an unwritten target: its term
            p.calc(name, p.column(2, 1), p.challenge(1))
        out.append(("tiny_" + name, p))
    b = Builder(B, k, ext_k)
    b.p.calc("mul", b.p.previous(), b.p.previous())
    out.append(("tiny_previous_both", b.p))
    b = Builder(B, k, ext_k)                                            # never reads `previous`: the old output must not leak in
    b.p.calc("mul", b.p.calc("add", b.p.column(0, 2), b.p.constant(EP.word(EP.CONST_WORDS[0]))), b.p.challenge(0))
    out.append(("tiny_no_previous", b.p))
    b = Builder(B, k, ext_k)
    b.p.calc("add", b.p.column(0, 0), b.p.previous())
    b.p.calc("store", b.p.column(3, -2))
    out.append(("tiny_store_rot_m2", b.p))
    return out


# (R, seed, fresh Horner steps).  The ring sizes 8 and 9 lie on both sides of the interpreter's 8 registers by INDEX count; scheduled,
# they need 6 and 8 slots.  By SLOT count (slot_plan below; tests/test_evalh_forms_cpu.py pins these figures): ring_10 with this seed
# needs 9 slots as scheduled -- exactly one spilled slot, acquired more than once -- and ring_40 spills many, two of them taken by a Horner
# step on a never-written index
RINGS = [(3, 1003, ()), (8, 1008, ()), (9, 1009, ()), (10, 1000, ()), (40, 1053, (50, 80))]


def forms(B, k=K, ext_k=EXT_K):
    """[(name, GraphProgram, n_columns, n_challenges)]"""
    out = [("ring_%d" % R, ring(B, R, seed, k=k, ext_k=ext_k, fresh_horner=fh)) for R, seed, fh in RINGS]
    out.append(("self_update", self_update(B, k, ext_k)))
    out.append(("operand_sweep", operand_sweep(B, k, ext_k)))
    out.append(("horner_mixed", horner_mixed(B, k, ext_k)))
    out += [("horner_first_" + f, horner_first(B, f, k, ext_k)) for f in ("column", "challenge", "previous")]
    out += [("dead_code", dead_code(B, k, ext_k)), ("dead_horner", dead_horner(B, k, ext_k))]
    out += tiny(B, k, ext_k)
    return [(n, p, N_COLUMNS, N_CHALLENGES) for n, p in out]


FORM_NAMES = ["ring_3", "ring_8", "ring_9", "ring_10", "ring_40", "self_update", "operand_sweep", "horner_mixed", "horner_first_column",
              "horner_first_challenge",
              "horner_first_previous", "dead_code", "dead_horner", "tiny_add", "tiny_sub", "tiny_mul", "tiny_square", "tiny_double",
              "tiny_negate", "tiny_store", "tiny_horner_step", "tiny_previous_both", "tiny_no_previous", "tiny_store_rot_m2"]
HAZARD_FORMS = ["ring_3", "ring_8", "ring_9", "ring_10", "ring_40", "self_update"]


# ---- refused: reads of intermediates no instruction has written ------------------------------------------------------------------------
def refused(B, k=K, ext_k=EXT_K):
    """[(name, GraphProgram, n_columns, n_challenges, by_validation)]: every call must fail with EZKL_ERR_INVALID.  by_validation: the
    operand check alone sees it (an index past n_intermediates); the others name a valid index that is not written when it is read"""
    out = []
    for q in (0, 1):
        b = Builder(B, k, ext_k)
        a = b.op("add", b.load(), b.load())
        ghost = b.new()
        b.op("mul", *((I(ghost), a) if q == 0 else (a, I(ghost))))
        out.append(("unwritten_operand_%d" % q, b.p, False))
    b = Builder(B, k, ext_k)
    ghost, t = b.new(), b.new()
    b.put(t, "horner_step", b.load(), I(ghost))                         # the target is unwritten too: the step is its term, the factor still counts
    b.op("add", I(t), b.load())
    out.append(("unwritten_horner_factor", b.p, False))
    b = Builder(B, k, ext_k)
    late = b.new()
    c = b.op("add", I(late), b.load())
    b.put(late, "store", b.load())                                      # its only write comes after the read
    b.op("add", c, I(late))
    out.append(("written_later", b.p, False))
    b = Builder(B, k, ext_k)
    a = b.op("add", b.load(), b.load())
    b.op("mul", a, I(b.p.n_intermediates + 3))
    out.append(("index_out_of_range", b.p, True))
    return [(n, p, N_COLUMNS, N_CHALLENGES, v) for n, p, v in out]


REFUSED_NAMES = ["unwritten_operand_0", "unwritten_operand_1", "unwritten_horner_factor", "written_later", "index_out_of_range"]


# ---- check kernel: a listed slot written three times ------------------------------------------------------------------------------------
def check_programs(B, k):
    """[(name, GraphProgram, slot)] for the mock prover's check kernel (k == ext_k), over two columns: column 0 (A) must be non-zero on
    every row, column 1 (Z) is zero except on the planted rows.  `last_zero`: the first two versions of the slot are non-zero on every
    row, the last one is non-zero exactly where Z is.  `last_nonzero`: the first two versions are zero everywhere, the last one as before.
    A kernel that tested any version but the last reports every row, or none"""
    out = []
    for name in ("last_zero", "last_nonzero"):
        p = B.GraphProgram(k, k)
        A, Z = p.column(0, 0), p.column(1, 0)
        s = p.n_intermediates
        p.n_intermediates += 1
        if name == "last_zero":
            p.calc("store", A, target=s)                                # A
            w = p.calc("add", I(s), I(s))                               # 2 A: a reader of the first version
            p.calc("mul", I(s), A, target=s)                            # A^2
            w = p.calc("mul", w, I(s))                                  # 2 A^3: never zero
        else:
            p.calc("sub", A, A, target=s)                               # 0
            w = p.calc("add", I(s), A)                                  # A
            p.calc("mul", I(s), w, target=s)                            # 0
            w = p.calc("add", w, I(s))                                  # A
        p.calc("mul", Z, w, target=s)                                   # zero exactly where Z is
        p.calc("add", I(s), w)                                          # the program goes on after the last write
        out.append((name, p, s))
    return out


# ---- hazards, found on the host --------------------------------------------------------------------------------------------------------
def reads(ins):
    """the intermediate indices an instruction reads (a Horner step reads its target)"""
    r = [int(ins[3 + 3 * q]) for q in range(1 if int(ins[0]) in UNARY else 2) if int(ins[2 + 3 * q]) == INTERMEDIATE]
    return r + [int(ins[1])] if int(ins[0]) == HORNER else r


def live(code):
    """live[i]: the value instruction i writes reaches the program's result"""
    need, out = {int(code[-1][1])}, [False] * len(code)
    for i in range(len(code) - 1, -1, -1):
        t = int(code[i][1])
        if t in need:
            out[i] = True
            need.discard(t)
            need.update(reads(code[i]))
    return out


def hazard_orders(code):
    """-> (war, waw): orders a scheduler without that edge could emit, each as (j, at, order): the program with the ADJACENT
    instructions i, i + 1 swapped, the instruction j whose value the swap changes, and its place `at` in the new order.
    war: i + 1 overwrites an index that i reads and does not read i's target (swapped, i reads the new value: j = i).
    waw: both write the same index and neither reads it (swapped, the first value stays: j = i + 1).
    No other dependency ties such a pair, so the swap breaks that one edge alone.  Pairs whose value cannot reach the result (no chain
    of reads leads there) or that write what was there anyway are left out"""
    code = [list(map(int, ins)) for ins in code]
    lv = live(code)
    war, waw = [], []
    for i in range(len(code) - 2):                     # the last instruction stays last
        a, b = code[i], code[i + 1]
        swapped = code[:i] + [b, a] + code[i + 2:]
        if a[1] != b[1] and b[1] in reads(a) and a[1] not in reads(b) and lv[i] and b[:5] != [6, b[1], INTERMEDIATE, b[1], 0]:
            war.append((i, i + 1, swapped))            # (a store of an index onto itself writes what was there)
        if a[1] == b[1] and a[1] not in reads(a) + reads(b) and lv[i + 1] and a != b:
            waw.append((i + 1, i + 1, swapped))
    return war, waw


def nudged(code, j, const_idx):
    """the program with the value instruction j writes changed (a non-zero constant added to it): if the result moves, that value matters"""
    code = [list(map(int, ins)) for ins in code]
    t = code[j][1]
    return code[:j + 1] + [[0, t, INTERMEDIATE, t, 0, CONST, const_idx, 0]] + code[j + 1:]


# ---- the slots a program takes -------------------------------------------------------------------------------------------------------
def slot_plan(code, n_reg=8):
    """allocate_slots of ezkl_amd/csrc/evalh.hip restated (value versions, a slot released after the last read of its value, lowest free
    slot first), to say what a form exercises: -> (slots used, slots of the Horner steps on never-written targets, number of times a
    slot >= n_reg -- one of the interpreter's spilled slots -- is acquired again).  It describes the inputs; no value is checked with it"""
    code = [list(map(int, ins)) for ins in code]
    n = len(code)
    cur, last_use, src_ver, tgt, fresh = {}, {}, {}, {}, []
    for i, ins in enumerate(code):
        if ins[0] == HORNER and ins[1] not in cur:
            ins[0] = 6                                 # its term alone: a store
            fresh.append(i)
        for q in range(1 if ins[0] in UNARY else 2):
            if ins[2 + 3 * q] == INTERMEDIATE:
                src_ver[i, q] = cur[ins[3 + 3 * q]]
                last_use[src_ver[i, q]] = i
        if ins[0] == HORNER:
            tgt[i] = cur[ins[1]]
            last_use[tgt[i]] = i
        else:
            cur[ins[1]] = tgt[i] = i
    last_use[tgt[n - 1]] = n
    slot, free, used, fresh_slots, again = {}, [], 0, [], 0

    def release(v):
        if slot.get(v, -1) >= 0:
            free.append(slot[v])
            slot[v] = -2
    for i, ins in enumerate(code):
        for q in range(1 if ins[0] in UNARY else 2):
            v = src_ver.get((i, q))
            if v is not None and v != tgt[i] and last_use[v] == i:
                release(v)
        if tgt[i] == i:
            if free:
                slot[i] = min(free)
                free.remove(slot[i])
                again += slot[i] >= n_reg
            else:
                slot[i], used = used, used + 1
            if i in fresh:
                fresh_slots.append(slot[i])
        if last_use.get(tgt[i], -1) <= i and last_use.get(tgt[i]) != n:
            release(tgt[i])
    return used, fresh_slots, again
