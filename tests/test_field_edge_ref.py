"""CPU side of the field-primitive edge tests: the reference of tests/field_edge_ref.py is itself checked here (operand lists against
the preconditions of the headers; the radix-2^29 product rule against the instruction-by-instruction interpreter of
tests/test_montmul29_asm.py on the whole operand list; canonical / cond_sub / is_zero_mod_p by their defining arithmetic), the probe's
name table is compared with the reference's, and the __host__ halves of Field<P> run on the same operands as a plain program under
UndefinedBehaviorSanitizer (tests/cpp/field_host_probe.cpp: no device, nothing loaded into the interpreter, no preload)."""
import os
import shutil
import subprocess

import pytest

import field_edge_ref as F
import test_montmul29_asm as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def test_probe_table_and_reference_name_the_same_primitives():
    """a primitive without a reference, or a reference without a primitive, fails here (the name query is host code)"""
    from ezkl_amd import backend as B
    table = B.field_probe_names()
    assert sorted(table) == F.names()
    for name in table:
        assert table[name] == tuple(F.shape(name)), name
    # what the issue's table asks for, spelled out once so that dropping a row from BOTH sides is noticed as well
    want32 = "add sub neg dbl reduce_once mul mul_inl sqr mul_lazy redc from_mont to_mont add_lazy sub_lazy reduce_2p inv".split()
    want29 = "unpack pack normalize mul mul_cold sqr sqr_cold canonical is_zero_mod_p".split()
    want29 += ["sub%d" % k for k in range(7)] + ["neg%d" % k for k in range(7)] + ["cond_sub%d" % k for k in range(4)]
    for f in ("fr", "fq"):
        assert all("%s.%s" % (f, n) in table for n in want32 + ["live_mul_inl", "live_mul_lazy"])
        assert all("%s29.%s" % (f, n) in table for n in want29 + ["live_mul", "live_sqr"])
    assert "fq29.mul2add" in table and "fq29.live_mul2add" in table and "fr29.mul2add" not in table


@pytest.mark.parametrize("name", F.names())
def test_operands_respect_the_preconditions(name):
    F.check_domain(name)
    ops, want, n_edge = F.case(name)
    arity, w_in, w_out = F.shape(name)
    assert len(ops) == arity and all(o.shape == (len(want), w_in) for o in ops) and want.shape[1] == w_out and 0 < n_edge <= len(want)


def test_edge_lists_hold_what_they_promise():
    for p in (F.FR, F.FQ):
        e = set(F.edge_words(p))
        assert {0, 1, p - 1, (p - 1) // 2, (p + 1) // 2, F.R256 % p, F.M32, F.M32 << 192, (1 << 253) - 1}.issubset(e)
        sums = {a + b for a in e for b in e}
        diffs = {a - b for a in e for b in e}
        assert {p - 1, p, p + 1}.issubset(sums) and {-1, 0, 1}.issubset(diffs)
        assert F.words32(p)[0] in e                                     # times the stored 1: first quotient digit 0xffffffff
        assert (F.words32(p)[0] * (-pow(p, -1, 1 << 32) % (1 << 32))) & F.M32 == F.M32
        assert {p, 2 * p - 1}.issubset(F.lazy_words(p, 2 * p)) and 2 * p not in F.lazy_words(p, 2 * p)
        assert {2 * p, 2 * p + 1, 4 * p - 1}.issubset(F.lazy_words(p, 4 * p)) and {F.R256 - 1, F.R256 - p}.issubset(F.any_words(p))
        v = set(F.values29(p))
        assert all({j * p, j * p + 1}.issubset(v) for j in range(170)) and (F.R261 - 1) in v and 169 * p < F.R261 < 170 * p


@pytest.mark.parametrize("field", ["fr29", "fq29"])
def test_reduction_rules_by_their_defining_arithmetic(field):
    p = F.MODS[field]
    for name, K in [("canonical", None)] + [("cond_sub%d" % k, 1 << k) for k in range(4)]:
        edge, rnd = F.int_rows("%s.%s" % (field, name))
        for (v,) in edge + rnd:
            x, r = F.value29(v), F.expected_words("%s.%s" % (field, name), (v,))
            y = F.value29(r)
            assert all(l <= F.M29 for l in r) and (x - y) % p == 0
            if K is None:
                assert 0 <= y < p
            else:
                assert (y == x - K * p and x >= K * p) or (y == x and x < K * p)
    multiples = {j * p for j in range(32)}
    edge, _ = F.int_rows(field + ".is_zero_mod_p")
    flags = [F.expected_words(field + ".is_zero_mod_p", r)[0] for r in edge]
    assert flags == [1 if F.value29(r[0]) in multiples else 0 for r in edge] and sum(flags) == 32
    # rows whose low limb is that of a multiple below 32 p although they are none: the limb-by-limb compare decides these
    p0inv = pow(p, -1, 1 << 29)
    assert sum(1 for r, f in zip(edge, flags) if not f and (r[0][0] * p0inv) & F.M29 < 32) >= 32 * 5
    for KI in range(7):
        for prim in ("sub%d" % KI, "neg%d" % KI):
            edge, rnd = F.int_rows("%s.%s" % (field, prim))
            for r in edge + rnd:
                got = F.value29(F.expected_words("%s.%s" % (field, prim), r))
                assert got == (F.value29(r[0]) if len(r) == 2 else 0) - F.value29(r[-1]) + (2 << KI) * p


@pytest.mark.parametrize("fn,case", [("mont_mul29_fr", "fr29.mul"), ("mont_mul29_fq", "fq29.mul"), ("mont_sqr29_fr", "fr29.sqr"),
                                     ("mont_sqr29_fq", "fq29.sqr"), ("mont_mul2add29_fq", "fq29.mul2add")])
def test_product_rule_agrees_with_the_interpreted_assembly(fn, case):
    """limbs29(redc(A B [+ C D], p, 261)), all nine limbs, on every row the device probe gets -- and no 64-bit column overflows"""
    lines = A.asm_of(fn)
    ops, want, _ = F.case(case)
    rows = [o.tolist() for o in ops]
    want = want.tolist()
    for i in range(len(want)):
        got = A.run(lines, {n: rows[k][i] for k, n in enumerate("abcd"[:len(rows)])})
        assert got == want[i], F.describe(case, ops, [got] * (i + 1), want, i)
    if not case.endswith("mul2add"):                                     # the out-of-line form: the same rows, the same words
        cold_ops, cold_want, _ = F.case(case + "_cold")
        assert cold_want.tolist() == want and all((x == y).all() for x, y in zip(cold_ops, ops))


def test_a_wrong_rule_shows_on_the_edge_rows_only():
    """the evidence that the edge lists carry the test: with `a > p` for `a >= p` in reduce_once the expectation changes on the one row
    a = p and on no random row; with `>` for `>=` in add_lazy on the rows a + b = 2p"""
    for field in ("fr", "fq"):
        p = F.MODS[field]
        edge, rnd = F.int_rows(field + ".reduce_once")
        wrong = lambda a: a - p if a > p else a
        assert [a for (a,) in edge if wrong(a) != F.reduce_once_rule(a, p)] == [p]
        assert not [a for (a,) in rnd if wrong(a) != F.reduce_once_rule(a, p)]
        edge, rnd = F.int_rows(field + ".add_lazy")
        hit = [(a, b) for a, b in edge if a + b == 2 * p]
        assert len(hit) >= 3 and not [1 for a, b in rnd if a + b == 2 * p]


def _hex(x):
    return "%064x" % x


@pytest.mark.skipif(HIPCC is None, reason="hipcc is not installed")
def test_host_halves_under_ubsan(tmp_path):
    exe, fin, fout = str(tmp_path / "field_host_probe"), str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    cmd = [HIPCC, "--offload-host-only", "-x", "hip", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=undefined", "-Xarch_host",
           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "field_host_probe.cpp"), "-o", exe, "-fsanitize=undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-6000:]
    want = []
    with open(fin, "w") as f:
        for field in ("fr", "fq"):
            p = F.MODS[field]
            for prim in F.TABLE32:
                edge, rnd = F.int_rows("%s.%s" % (field, prim))
                for ops in edge + rnd:
                    f.write("%s.%s %s\n" % (field, prim, " ".join(_hex(x) for x in ops)))
                    want.append(("%s.%s" % (field, prim), ops, F.host_expected32(prim, p, *ops)))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stderr[-6000:]
    got = open(fout).read().split("\n")[:-1]
    assert len(got) == len(want)
    for line, (name, ops, exp) in zip(got, want):
        assert line == "%s %s" % (name, _hex(exp)), "%s(%s): host gave %s, expected %s" % (name, ", ".join(_hex(x) for x in ops), line.split()[-1], _hex(exp))
