"""Quotient-sweep programs that sit on the limits of the radix-2^29 code generator (ezkl_amd/csrc/evalh.hip, jit_source_r29), shared by
tests/test_evalh29_model.py (the integer model of the generated source, CPU) and tests/test_gpu_evalh_bounds.py (the kernels, GPU).

The generator tracks for every value a bound alpha (value < alpha p) and a limb looseness L (limbs < L 2^29); a load has alpha 32, L 1.
Values with a small alpha come from products: load x load -> 8, 8 x load -> 3, 3 x load -> 2 (alpha_a alpha_b / 169 rounded up, plus 1),
so sums of 32, 8, 3 and 2 reach every alpha >= 2 exactly.  Every builder below says which limit it reaches."""
import numpy as np


N_COLUMNS = 4
N_CHALLENGES = 3
K, EXT_K = 3, 5
R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
# constant words (Montgomery forms as stored) at the edges of [0, p): the program's constants are these raw words
CONST_WORDS = [R - 1, (R - 1) // 2, (R + 1) // 2, R - 2, 1, (1 << 253) + 0x1234567, 0]


def word(x):
    return np.frombuffer(int(x).to_bytes(32, "little"), np.uint64).copy()


class Builder:
    """a GraphProgram with loads that cycle over columns (rotations -2..2), challenges, constants and `previous`"""

    def __init__(self, B, k=K, ext_k=EXT_K):
        self.B = B
        self.p = B.GraphProgram(k, ext_k)
        self.i = 0
        for c in CONST_WORDS:
            self.p.constant(word(c))

    def load(self):
        j = self.i
        self.i += 1
        if j % 7 == 5:
            return self.p.challenge(j % N_CHALLENGES)
        if j % 7 == 6:
            return self.p.constant(word(CONST_WORDS[(j // 7) % len(CONST_WORDS)]))
        return self.p.column(j % N_COLUMNS, (j % 5) - 2)

    def op(self, name, a, b=None):
        return self.p.calc(name, a) if b is None else self.p.calc(name, a, b)

    def loads_sum(self, n):
        """alpha 32 n, L n (n <= 5)"""
        v = self.load()
        for _ in range(n - 1):
            v = self.op("add", v, self.load())
        return v

    def atom(self, a):
        """one value with alpha exactly a in {32, 8, 3, 2}, L 1"""
        if a == 32:
            return self.load()
        v = self.op("mul", self.load(), self.load())            # 8
        if a == 8:
            return v
        v = self.op("mul", v, self.load())                      # 3
        if a == 3:
            return v
        assert a == 2
        return self.op("mul", v, self.load())

    def with_alpha(self, a):
        """a value whose alpha is exactly a (2 <= a <= 160): a sum of atoms, largest first"""
        parts = []
        while a:
            for x in (32, 8, 3, 2):
                if a - x >= 0 and a - x != 1:
                    parts.append(x)
                    a -= x
                    break
        v = self.atom(parts[0])
        for x in parts[1:]:
            v = self.op("add", v, self.atom(x))
        return v

    def done(self, v):
        """the program's result is the last instruction's target: make v that"""
        if self.p.code[-1][1] != v[1]:
            self.op("store", v)
        return self.p


# ---- (a) add and doubling chains onto alpha 160 and L 6 ----------------------------------------------------------------------------
def fam_a(B):
    out = []
    b = Builder(B)                                     # five loads: alpha 160, L 5 -- the value the final product takes at its largest
    out.append(("a_five_loads", b.done(b.loads_sum(5))))
    b = Builder(B)                                     # doublings: 32 -> 64 -> 128 (L 4), + a doubled product (16, L 2) = 144, L 6;
    x = b.op("double", b.op("double", b.load()))      # then a product with L_a L_b = 6 at alpha beta = 4608
    y = b.op("add", x, b.op("double", b.atom(8)))
    out.append(("a_double_to_L6", b.done(b.op("mul", y, b.load()))))
    b = Builder(B)                                     # 160 exactly with L 6 (4 loads + 3 products of 8 + 2 ... ), doubled once more
    v = b.op("add", b.loads_sum(4), b.op("add", b.atom(8), b.atom(8)))
    v = b.op("add", v, b.atom(8))                      # 152, L 7 -> one carry pass on the way
    v = b.op("add", v, b.atom(8))                      # 160
    out.append(("a_sum_to_160", b.done(b.op("double", v))))
    return out


# ---- (b) every sub / neg borrow K, subtrahend at both ends of its band ---------------------------------------------------------------
BANDS = [(4, 2), (4, 3), (8, 4), (8, 7), (16, 8), (16, 15), (32, 16), (32, 31), (64, 32), (64, 63), (128, 64), (128, 127)]


def fam_b(B):
    """K = 2 needs a subtrahend with alpha <= 1, which no value has (a product is >= 2 p): the smallest borrow used is 4 p"""
    b = Builder(B)
    outs = []
    for K, a in BANDS:
        sub = b.op("sub", b.with_alpha(160 - K), b.with_alpha(a))     # the minuend as large as the borrow allows without a reduction
        outs.append(b.op("mul", sub, b.load()))
        outs.append(b.op("mul", b.op("negate", b.with_alpha(a)), b.load()))
    acc = outs[0]
    for v in outs[1:]:
        acc = b.op("add", acc, v)
    out = [("b_sub_neg_bands", b.done(acc))]
    b = Builder(B)                                     # alpha 160 > 127, L 5: the subtrahend is carried and reduced, then K = 4
    out.append(("b_sub_reduce", b.done(b.op("sub", b.load(), b.loads_sum(5)))))
    b = Builder(B)                                     # K = 128 and 64 from loads: the bound alpha p is met to within 32 (p - 1) < 32 p
    out.append(("b_neg_loads", b.done(b.op("add", b.op("negate", b.loads_sum(2)), b.op("negate", b.load())))))
    b = Builder(B)
    out.append(("b_sub_loads", b.done(b.op("add", b.op("sub", b.load(), b.loads_sum(2)), b.op("sub", b.load(), b.load())))))
    return out


# ---- (c) products on the limb and alpha limits ---------------------------------------------------------------------------------------
def fam_c(B, k=K, ext_k=EXT_K):
    b = Builder(B, k, ext_k)
    loose3 = b.op("sub", b.load(), b.atom(8))                           # alpha 48, L 3 by the generator's count (the SUBC limbs stay < 2.98)
    loose2 = b.op("add", b.load(), b.load())                            # alpha 64, L 2
    p6 = b.op("mul", loose3, loose2)                                    # L_a L_b = 6, 3072
    under = b.op("mul", b.with_alpha(156), b.load())                    # 4992: no reduction
    over = b.op("mul", b.with_alpha(157), b.load())                     # 5024: one reduction first
    sq = b.op("square", loose2)                                         # a loose-2 square: 4096
    sq3 = b.op("square", b.op("add", loose2, b.load()))                 # L 3: a carry pass first
    pp = b.op("mul", b.op("mul", p6, under), b.op("mul", over, sq))     # products of products
    v = b.op("add", b.op("add", pp, sq3), b.op("mul", loose3, loose3))  # loose-3 x loose-3: a carry pass on one side
    out = [("c_products", b.done(v))]
    b = Builder(B)                                     # a product over 5000 is reduced first; its result is a subtrahend (K from its alpha)
    out.append(("c_product_reduce", b.done(b.op("sub", b.load(), b.op("mul", b.with_alpha(157), b.load())))))
    b = Builder(B)                                     # three loads (96, L 3) x three products (24, L 3): limbs of 3 full units on both
    x = b.op("add", b.op("add", b.atom(8), b.atom(8)), b.atom(8))       # sides, 9 > 6 -- the carry pass keeps a column at 9 x 3 x 2^58 + ...
    out.append(("c_loose3_squared", b.done(b.op("mul", b.loads_sum(3), x))))     # (without it 81 x 2^58 would overflow), alpha beta = 2304
    b = Builder(B)                                     # (78, L 5) x (64, L 2): one carry pass, and alpha beta = 4992 needs no reduction
    x = b.op("add", b.op("add", b.loads_sum(2), b.atom(8)), b.op("add", b.atom(3), b.atom(3)))
    out.append(("c_mul_normalize", b.done(b.op("mul", x, b.op("add", b.load(), b.load())))))
    return out


# ---- (d) Horner -------------------------------------------------------------------------------------------------------------------
def fam_d(B, n_terms=64):
    b = Builder(B)
    factor = b.op("add", b.load(), b.op("mul", b.load(), b.load()))   # an intermediate: alpha 40, L 2
    terms = []
    for i in range(n_terms):
        t = b.atom(8)
        for _ in range(4):
            t = b.op("add", t, b.atom(8) if i % 2 else b.atom(3))         # L 5 sums
        terms.append(t)
    acc = b.p.horner(b.p.previous(), terms, factor)                      # store of previous, then the steps
    fresh = b.p.n_intermediates                                            # a Horner step on a target never written: 0 * factor + term
    b.p.n_intermediates += 1
    b.p.calc("horner_step", terms[0], factor, target=fresh)
    b.p.calc("horner_step", terms[1], b.load(), target=fresh)
    return [("d_horner", b.done(b.op("add", acc, (B.INTERMEDIATE, fresh, 0))))]


# ---- (e) one version as both operands -----------------------------------------------------------------------------------------------
def fam_e(B):
    b = Builder(B)
    v = b.op("add", b.loads_sum(3), b.atom(8))                 # alpha 104, L 4
    s = b.op("add", v, v)                                        # add(v, v): both sides loose
    d = b.op("sub", v, v)
    m = b.op("mul", v, v)
    n = b.op("negate", b.op("negate", v))
    w = b.op("sub", b.load(), s)
    return [("e_same_operand", b.done(b.op("add", b.op("add", b.op("mul", d, m), n), w)))]


# ---- (f) a final value with alpha in [150, 169] -------------------------------------------------------------------------------------
def fam_f(B):
    out = []
    b = Builder(B)
    out.append(("f_sub_160", b.done(b.op("sub", b.load(), b.loads_sum(2)))))          # 32 + 128
    b = Builder(B)
    out.append(("f_sum_152", b.done(b.with_alpha(152))))
    b = Builder(B)
    t = b.p.horner(b.p.previous(), [b.with_alpha(150)], b.load())                     # 150 + a product of 1024 -> 157
    out.append(("f_horner_157", b.done(t)))
    return out


# programs of families (b) and (c) in which EVERY emitted line of a kind sits on a limit: removing any carry pass ("normalize") or
# reduction ("reduce"), or lowering any borrow ("sub", "neg") by one step, breaks a precondition (tests/test_evalh29_model.py).  Elsewhere
# some emitted lines are only conservative -- e.g. the second carry pass of a version used as both operands
TIGHT = {"b_sub_reduce": ("reduce", "sub"), "b_neg_loads": ("normalize", "neg"), "b_sub_loads": ("normalize", "sub"),
         "c_product_reduce": ("normalize", "reduce", "sub"), "c_mul_normalize": ("normalize",), "c_loose3_squared": ("normalize",)}


def families(B):
    """[(name, GraphProgram)] of families (a) .. (f)"""
    return fam_a(B) + fam_b(B) + fam_c(B) + fam_d(B) + fam_e(B) + fam_f(B)


def random_program(B, seed, ninstr, k=9, ext_k=11, ncols=12):
    """the random DAG of tests/test_gpu_misc.py (_random_program) with its own generator"""
    import test_gpu_misc as TG
    return TG._random_program(B, np.random.default_rng(seed), k, ext_k, ncols, ninstr)


# ---- the quotient programs of real circuits: only slot indices matter, so placeholders stand in for every coset handle ------------------
def quotient_program(cs):
    """-> (GraphProgram, number of columns, number of challenges) of plonk.quotient_program for `cs`"""
    from types import SimpleNamespace
    from ezkl_amd import plonk as P
    pk = SimpleNamespace(fixed_cosets=[None] * cs.n_fixed, sigma_cosets=[None] * len(cs.perm), l0=None, l_last=None, l_active=None,
                         x_coset=None)
    nl = len(cs.lookups)
    prog, cols, chal = P.quotient_program(cs, pk, [None] * cs.n_advice, [None] * cs.n_chunks, 5, 7, 11, 13, [None] * nl, [None] * nl,
                                          [None] * cs.n_instance, [17] * cs.n_challenges)
    return prog, len(cols), len(chal)


def circuit_programs():
    """[(name, GraphProgram, n_columns, n_challenges)]: the k = 6 ezkl fixture, a two-layer MLP and the einsum / transformer-surrogate unit"""
    import fixture_k6 as FX
    from ezkl_amd import ezkl_layout as EL
    out = [("q_fixture_k6",) + quotient_program(FX.load()["cs"])]
    mlp = EL.MlpCircuit(8, 2, [[[1, -2, 0], [3, 0, 1], [0, 1, -1]]] * 2, [[1, 0, -1]] * 2, 128, 2)
    out.append(("q_mlp",) + quotient_program(mlp.keygen_inputs([2, -1, 3])[0]))
    sur = EL.TransformerSurrogateCircuit(10, blocks=2, d=4, einsum_len=3, decomp_base=16, lookup_max=(1 << 10) // 16)
    out.append(("q_surrogate",) + quotient_program(sur.build(tiles=1)["cs"]))
    return out
