#!/usr/bin/env python3
"""Integer model of the quotient-sweep kernel that the radix-2^29 generator emits (ezkl_amd/csrc/evalh.hip, jit_source_r29).

The model reads the generated source itself (EZKL_HIP_JIT_DUMP: the exact text hiprtc compiles) and runs its straight-line body in one of
two modes, with every 32- / 64-bit register checked by the primitives of tools/ntt29_model.py:

  * concrete: one row on given words; the packed result must equal a plain big-int evaluation of the program (eval_program below);
  * worst case: every register carries an upper bound per limb and on its value (lower bound 0), propagated the way the hardware would
    in the worst case.  If this mode passes a source, the kernel cannot overflow a register or break a precondition of field29.hpp on any
    canonical input: the product's columns stay below 2^64, every sub / neg borrows enough, every carry pass gets limbs below 2^32 - 8,
    and the value handed to the final conditional subtraction is below 2p.

The body has a fixed set of line shapes (see LINE_SHAPES); any other line is an error."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ntt29_model as M  # noqa: E402

P = M.P
M29 = M.M29
R256 = 1 << 256
PL = M.limbs29(P)
ONE = M.limbs29(M.R261 % P)                 # Fr29::one(): 2^261 mod p, the Montgomery one of R' = 2^261
C_R256 = M.limbs29(R256 % P)                # Fr29::unpack(Fr::one()): 2^256 mod p, turns R' into R in the final product
CSUB = M.CSUB_P                             # Fr29C::CSUB[0] = 2^261 - p
SUBC = M.SUBC                               # K p with 2^29 lent to every lower limb, K = 2 << KI
LOAD_TOP = (P - 1) >> 227                   # top limb of a canonical word after the 5-bit shift: 0x060c89ce


def K_of(ki):
    assert 0 <= ki <= 6, "sub / neg index out of range: %d" % ki
    return 2 << ki


def ld29(w):
    """the generated ld29: a word w < 2^256 (x R) unpacked with a 5-bit shift -> 32 w = x 2^261, limbs 0..7 of 29 bits, limb 8 = w >> 227"""
    assert 0 <= w < R256
    return M.limbs29(w << 5)


def neg(b, K):
    """Fr29::neg<KI>: K p - b; b normalized and < (K - 1) p"""
    assert all(x <= M29 for x in b[:8]) and M.value(b) < (K - 1) * P, "neg: operand not normalized or too large for K = %d" % K
    out = []
    for c, x in zip(SUBC[K], b):
        assert c - x >= 0, "limb difference went negative"
        out.append(M.u32(c - x))
    return out


# ---- the source -------------------------------------------------------------------------------------------------------------------
_OPND = r"(v\d+|ld29\(cols\[\d+\] \+ \(\(r \+ \d+u\) & ne_mask\)\)|ld29\(consts \+ \d+\)|ld29\(chal \+ \d+\)|ld29\(out \+ r\))"
_MUL = r"Fr29::(?:mul|mul_cold)"
LINE_SHAPES = [
    ("add", re.compile(r"f29_t v(\d+) = Fr29::add\(%s, %s\);$" % (_OPND, _OPND))),
    ("sub", re.compile(r"f29_t v(\d+) = Fr29::sub<(\d)>\(%s, %s\);$" % (_OPND, _OPND))),
    ("neg", re.compile(r"f29_t v(\d+) = Fr29::neg<(\d)>\(%s\);$" % _OPND)),
    ("mul", re.compile(r"f29_t v(\d+) = %s\(%s, %s\);$" % (_MUL, _OPND, _OPND))),
    ("copy", re.compile(r"f29_t v(\d+) = %s;$" % _OPND)),
    ("normalize", re.compile(r"v(\d+) = Fr29::normalize\(v(\d+)\);$")),
    ("reduce", re.compile(r"v(\d+) = %s\(v(\d+), c_one\);$" % _MUL)),
    ("horner", re.compile(r"v(\d+) = Fr29::add\(%s\(v(\d+), %s\), %s\);$" % (_MUL, _OPND, _OPND))),
    ("store", re.compile(r"st_fe\(out \+ r, Fr29::pack\(Fr29::cond_sub<0>\(%s\(v(\d+), c_r256\)\)\)\);$" % _MUL)),
    # the check kernel of the mock prover (ezkl_hip_eval_check_dev): slot's value reduced as the store's is, then compared with zero
    ("check", re.compile(r"ezkl_report\(!Fr::is_zero\(Fr29::pack\(Fr29::cond_sub<0>\(%s\(v(\d+), c_r256\)\)\)\), (\d+)u, r, rec, cap, count\);$" % _MUL)),
    ("barrier", re.compile(r"(?:asm volatile\(\"\" ::: \"memory\"\)|__builtin_amdgcn_sched_barrier\(0\));$")),
]
# what the model's ld29 / constants assume about the preamble of the generated file
_PREAMBLE = ["r.v[0] = (w.v[0] << 5) & M29;", "const int bit = 29 * i - 5, word = bit >> 5, sh = bit & 31;",
             "r.v[i] = (sh ? __builtin_amdgcn_alignbit(hi, lo, sh) : lo) & M29;", "r.v[8] = w.v[7] >> 3;",
             "const f29_t c_one = Fr29::one();", "const f29_t c_r256 = Fr29::unpack(Fr::one());"]
_LOOP = "for (uint32_t r = tid; r <= ne_mask; r += T) {"
_LOOP_CHECK = "for (uint32_t r = row_lo + tid; r < row_hi; r += T) {"


def body(src):
    """the statements of the row loop, each as (line number, stripped text)"""
    lines = src.splitlines()
    for s in _PREAMBLE:
        assert s in src, "generated preamble changed: %r not found" % s
    start = [i for i, l in enumerate(lines) if l.strip() in (_LOOP, _LOOP_CHECK)]
    assert len(start) == 1, "row loop not found"
    out = []
    for i in range(start[0] + 1, len(lines)):
        t = lines[i].strip()
        if t == "}":
            return out
        out.append((i + 1, t))
    raise AssertionError("row loop not closed")


def parse(src):
    """-> [(kind, groups, line number)]; raises on any line outside LINE_SHAPES"""
    prog = []
    for ln, t in body(src):
        for kind, rx in LINE_SHAPES:
            m = rx.match(t)
            if m:
                if kind in ("normalize", "reduce", "horner"):
                    assert m.group(1) == m.group(2), "line %d: in-place update of another variable: %s" % (ln, t)
                if kind != "barrier":
                    prog.append((kind, m.groups(), ln))
                break
        else:
            raise AssertionError("line %d: not a shape the model knows: %s" % (ln, t))
    n_store, n_check = sum(k == "store" for k, _, _ in prog), sum(k == "check" for k, _, _ in prog)
    if n_check:                                        # a check kernel: no store, every listed slot tested once
        assert n_store == 0, "a check kernel stores nothing"
        slots = [int(g[1]) for k, g, _ in prog if k == "check"]
        assert len(set(slots)) == len(slots), "a slot is checked twice"
    else:
        assert prog and prog[-1][0] == "store" and n_store == 1, "the body must end in its one store"
    return prog


# ---- the two domains --------------------------------------------------------------------------------------------------------------
class Concrete:
    """registers are the 9 limbs of one row; every operation is the checked primitive of ntt29_model"""

    def __init__(self, cols, consts, chal, prev):
        self.cols, self.consts, self.chal, self.prev = cols, consts, chal, prev

    def load(self, kind, idx):
        w = {"col": lambda: self.cols[idx], "const": lambda: self.consts[idx], "chal": lambda: self.chal[idx], "prev": lambda: self.prev}[kind]()
        return ld29(w)

    add = staticmethod(M.add)
    normalize = staticmethod(M.normalize)
    mul = staticmethod(M.mont_mul)

    @staticmethod
    def sub(a, b, K):
        return M.sub(a, b, K)

    @staticmethod
    def neg(b, K):
        return neg(b, K)

    @staticmethod
    def const(limbs):
        return list(limbs)

    @staticmethod
    def final(x):
        y = M.mont_mul(x, C_R256)
        assert M.value(y) < 2 * P, "value before the final conditional subtraction is not below 2p"
        return M.pack(M.cond_sub_p(y))


class Bound:
    """registers are (limb maxima, value maximum); every value has lower bound 0"""

    @staticmethod
    def eff(x):
        lim, vmax = x
        return [min(l, vmax >> (29 * i)) for i, l in enumerate(lim)]

    def load(self, kind, idx):
        return ([M29] * 8 + [LOAD_TOP], 32 * (P - 1))

    @staticmethod
    def const(limbs):
        return (list(limbs), M.value(limbs))

    def add(self, a, b):
        return ([M.u32(x + y) for x, y in zip(self.eff(a), self.eff(b))], a[1] + b[1])

    def _borrow_ok(self, b, K, what):
        lb = self.eff(b)
        assert all(x <= M29 for x in lb[:8]), "%s<K=%d>: operand may not be normalized" % (what, K)
        assert b[1] < (K - 1) * P, "%s<K=%d>: operand may reach %.3f p, needs < %d p" % (what, K, b[1] / P, K - 1)
        for c, x in zip(SUBC[K], lb):
            assert c >= x, "%s<K=%d>: a limb difference may go negative" % (what, K)

    def sub(self, a, b, K):
        self._borrow_ok(b, K, "sub")
        return ([M.u32(x + c) for x, c in zip(self.eff(a), SUBC[K])], a[1] + K * P)

    def neg(self, b, K):
        self._borrow_ok(b, K, "neg")
        return (list(SUBC[K]), K * P)

    def normalize(self, a):
        r = self.eff(a)
        for i in range(8):
            assert r[i] < (1 << 32) - 8, "normalize: limb %d may reach %#x" % (i, r[i])
            r[i + 1] = M.u32(r[i + 1] + (r[i] >> 29))
            r[i] = min(r[i], M29)
        return (r, a[1])

    def mul(self, a, b):
        """the column structure of mont_mul29_fr on the limb maxima, with every m_i at 2^29 - 1"""
        la, lb = self.eff(a), self.eff(b)
        acc = 0
        for k in range(17):
            for i in range(max(0, k - 8), min(k, 8) + 1):
                acc = M.u64(acc + M.u32(la[i]) * M.u32(lb[k - i]))
            for i in (range(0, k) if k < 9 else range(k - 8, 9)):
                acc = M.u64(acc + M29 * PL[k - i])
            if k < 9:
                acc = M.u64(acc + M29 * PL[0])
            acc >>= 29
        vmax = (a[1] * b[1] + (M.R261 - 1) * P) >> 261
        return ([M29] * 8 + [min(M.u32(acc), vmax >> 232)], vmax)

    def final(self, x):
        y = self.mul(x, self.const(C_R256))
        assert all(l <= M29 for l in self.eff(y)[:8])
        assert y[1] < 2 * P, "value before the final conditional subtraction may reach %.4f p" % (y[1] / P)
        return y


def run(src, dom):
    """execute the generated body in a domain; returns what `final` returns plus the largest value bound seen (Bound) or None"""
    prog = parse(src)
    regs = {}
    peak = [0]

    def opnd(t):
        if t.startswith("v"):
            assert t in regs, "read of %s before it is defined" % t
            return regs[t]
        m = re.match(r"ld29\(cols\[(\d+)\]", t)
        if m:
            return dom.load("col", int(m.group(1)))
        m = re.match(r"ld29\(consts \+ (\d+)\)", t)
        if m:
            return dom.load("const", int(m.group(1)))
        m = re.match(r"ld29\(chal \+ (\d+)\)", t)
        if m:
            return dom.load("chal", int(m.group(1)))
        assert t == "ld29(out + r)"
        return dom.load("prev", 0)

    def define(name, val, fresh):
        assert (name not in regs) == fresh, "%s: %s" % ("redefinition" if fresh else "update of an undefined variable", name)
        regs[name] = val
        if isinstance(dom, Bound):
            peak[0] = max(peak[0], val[1])

    checks = []
    for kind, g, ln in prog:
        try:
            if kind == "add":
                define("v" + g[0], dom.add(opnd(g[1]), opnd(g[2])), True)
            elif kind == "sub":
                define("v" + g[0], dom.sub(opnd(g[2]), opnd(g[3]), K_of(int(g[1]))), True)
            elif kind == "neg":
                define("v" + g[0], dom.neg(opnd(g[2]), K_of(int(g[1]))), True)
            elif kind == "mul":
                define("v" + g[0], dom.mul(opnd(g[1]), opnd(g[2])), True)
            elif kind == "copy":
                define("v" + g[0], opnd(g[1]), True)
            elif kind == "normalize":
                define("v" + g[0], dom.normalize(opnd("v" + g[0])), False)
            elif kind == "reduce":
                define("v" + g[0], dom.mul(opnd("v" + g[0]), dom.const(ONE)), False)
            elif kind == "horner":
                t = "v" + g[0]
                define(t, dom.add(dom.mul(opnd(t), opnd(g[2])), opnd(g[3])), False)
            elif kind == "check":
                checks.append((int(g[1]), dom.final(opnd("v" + g[0]))))
            else:
                return dom.final(opnd("v" + g[0])), (peak[0] if isinstance(dom, Bound) else None)
        except AssertionError as e:
            raise AssertionError("line %d (%s): %s" % (ln, kind, e)) from None
    if checks:
        return checks, (peak[0] if isinstance(dom, Bound) else None)
    raise AssertionError("unreachable")


def worst_case(src):
    """worst-case mode: raises AssertionError on the first possible violation; returns the largest value bound, in units of p"""
    _, peak = run(src, Bound())
    return peak / P


def concrete(src, cols, consts, chal, prev):
    """concrete mode: one row.  cols[i] is the word every rotation of column i reads in this row (the dumped source is generated with
    every rotation offset at 0); words are the Montgomery forms x 2^256 mod p as integers.  Returns the 256-bit word the kernel stores."""
    return run(src, Concrete(cols, consts, chal, prev))[0]


def concrete_checks(src, cols, consts, chal):
    """concrete mode of a check kernel: one row -> {slot: the 256-bit word its value reduces to} (the kernel reports the slot if non-zero)"""
    return dict(run(src, Concrete(cols, consts, chal, 0))[0])


# ---- the plain big-int evaluation of a program ------------------------------------------------------------------------------------
RINV = pow(R256, -1, P)
OPS = dict(add=0, sub=1, mul=2, square=3, double=4, negate=5, store=6, horner_step=7)
CONST, INTERMEDIATE, COLUMN, CHALLENGE, PREVIOUS = range(5)


def eval_program(code, consts, chal, prev, read):
    """the program (rows of 8 words, ezkl_program_t) over Fr, in its own order: read(column, rotation index) -> word.  Words are
    Montgomery forms and may be any 256-bit value (their residue counts); returns the canonical Montgomery word of the result."""
    vals = {}

    def src(kind, idx, rot):
        if kind == CONST:
            return consts[idx] * RINV % P
        if kind == INTERMEDIATE:
            return vals[idx]
        if kind == COLUMN:
            return read(idx, rot) * RINV % P
        if kind == CHALLENGE:
            return chal[idx] * RINV % P
        assert kind == PREVIOUS
        return prev * RINV % P

    last = None
    for ins in code:
        op, t = int(ins[0]), int(ins[1])
        a = src(*[int(x) for x in ins[2:5]])
        unary = op in (OPS["square"], OPS["double"], OPS["negate"], OPS["store"])
        b = None if unary else src(*[int(x) for x in ins[5:8]])
        if op == OPS["add"]:
            v = a + b
        elif op == OPS["sub"]:
            v = a - b
        elif op == OPS["mul"]:
            v = a * b
        elif op == OPS["square"]:
            v = a * a
        elif op == OPS["double"]:
            v = 2 * a
        elif op == OPS["negate"]:
            v = -a
        elif op == OPS["store"]:
            v = a
        else:
            v = vals.get(t, 0) * b + a                       # horner_step: target = target * factor + term
        vals[t] = v % P
        last = t
    return vals[last] * R256 % P
