"""The radix-2^29 quotient-sweep generator (ezkl_amd/csrc/evalh.hip, jit_source_r29) checked on the source it emits: tools/evalh29_model.py
runs the dumped kernel body with every register bounded in the worst case, and on concrete rows against a big-int evaluation of the
program.  Host only: the library hands over the source it would compile (GraphProgram.generated_source), no hiprtc compile and no GPU needed.
The kernels themselves run on these programs in tests/test_gpu_evalh_bounds.py."""
import os
import random
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
import evalh_programs as EP

sys.path.insert(0, os.path.join(ROOT, "tools"))
import evalh29_model as E  # noqa: E402

P = E.P
EZKL_ERR_INVALID = -3            # include/ezkl_hip.h


def _word(a):
    return int.from_bytes(np.ascontiguousarray(a, np.uint64).tobytes(), "little")


def _programs():
    """[(name, GraphProgram, n_columns, n_challenges)]: families (a) .. (f), three random DAGs (one of 1200 instructions) and the quotient
    programs of three circuits"""
    from ezkl_amd import backend as B
    out = [(n, p, EP.N_COLUMNS, EP.N_CHALLENGES) for n, p in EP.families(B)]
    for seed, n in ((1, 300), (2, 300), (5, 1200)):
        out.append(("random_%d_%d" % (seed, n), EP.random_program(B, seed, n), 12, 3))
    return out + EP.circuit_programs()


@pytest.fixture(scope="module")
def dumps():
    """every program lowered once per radix-2^29 variant (EZKL_EVALH_R29=2: the product as a call, =1: inline), as the library generates
    it (GraphProgram.generated_source: the text ezkl_hip_eval_h_check would hand hiprtc, without the compile):
    {(name, variant): (source, program, n_columns, n_challenges)}"""
    out = {}
    mp = pytest.MonkeyPatch()
    try:
        for name, prog, nc, nch in _programs():
            for variant in ("2", "1"):
                mp.setenv("EZKL_EVALH_R29", variant)
                out[(name, variant)] = (prog.generated_source(nc), prog, nc, nch)
    finally:
        mp.undo()
    return out


def test_generated_source_is_what_check_compiles_dumps(monkeypatch, tmp_path):
    """the source the model reads is the one hiprtc compiles: the same text as the EZKL_HIP_JIT_DUMP of the compile check"""
    from ezkl_amd import backend as B
    prog = dict(EP.fam_c(B))["c_products"]
    for variant in ("2", "1"):
        monkeypatch.setenv("EZKL_EVALH_R29", variant)
        monkeypatch.setenv("EZKL_HIP_JIT_DUMP", str(tmp_path / "s.hip"))
        prog.check_compiles(EP.N_COLUMNS)
        assert open(tmp_path / "s.hip").read() == prog.generated_source(EP.N_COLUMNS)


def test_constants_are_the_generated_ones():
    src = open(os.path.join(ROOT, "ezkl_amd", "csrc", "montmul29_gen.hpp")).read()
    fr = src[src.index("struct Fr29C"):]

    def rows(tag):
        body = fr[fr.index(tag):]
        return [[int(x.rstrip("u"), 16) for x in m.split(", ")] for m in re.findall(r"\{(0x[^{}]*)\}", body)]
    assert rows("SUBC[7][9]")[:7] == [E.SUBC[2 << ki] for ki in range(7)]
    assert rows("CSUB[4][9]")[0] == E.CSUB
    assert rows("ONE[9]")[0] == E.ONE
    assert rows("P[9]")[0] == E.PL
    hdr = open(os.path.join(ROOT, "ezkl_amd", "csrc", "bn254_constants.h")).read()
    one = re.search(r"#define BN32_FR_R_INIT \{([^}]*)\}", hdr).group(1)
    r256 = sum(int(x.strip().rstrip("u"), 16) << (32 * i) for i, x in enumerate(one.split(",")))
    assert E.C_R256 == E.M.unpack(r256) and r256 == (1 << 256) % P        # c_r256 = Fr29::unpack(Fr::one())
    assert E.LOAD_TOP == 0x060c89ce


def test_load_is_the_shifted_word():
    """ld29 as generated: the 8 words shifted by 5 bits into 9 limbs of 29 -- a representative of x 2^261 for the word x 2^256"""
    for w in (0, 1, P - 1, (1 << 253) + 12345, (1 << 256) - 1):
        v = E.ld29(w)
        assert E.M.value(v) == 32 * w and all(x <= E.M29 for x in v[:8]) and v[8] == w >> 227


def test_worst_case_holds_for_every_program(dumps):
    peaks = {}
    for (name, variant), (src, _, _, _) in dumps.items():
        peaks[(name, variant)] = E.worst_case(src)
        if variant == "1":
            assert src == dumps[(name, "2")][0].replace("Fr29::mul_cold(", "Fr29::mul("), name
            assert "mul_cold" not in src
    # the families reach the limits they were built for: each of these programs holds a value bounded by 160 p (alpha 160)
    for n in ("a_five_loads", "b_sub_neg_bands", "e_same_operand", "f_sub_160"):
        assert peaks[(n, "2")] >= 159.9, n


def _rows(rnd, n_cols, n_consts, n_chal, n=8):
    """rows of extreme words: all p - 1, all 0, all in [2^253, p), and mixes with 1, p - 2, (p +- 1) / 2 and uniform words"""
    special = [0, 1, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2]
    pick = [lambda: P - 1, lambda: 0, lambda: rnd.randrange(1 << 253, P)]
    out = []
    for i in range(n):
        if i < 3:
            f = pick[i]
        else:
            f = lambda: rnd.choice(special) if rnd.random() < 0.5 else rnd.randrange(P)         # noqa: E731
        out.append(([f() for _ in range(n_cols)], [f() for _ in range(n_chal)], f()))
    return out


def test_concrete_rows_equal_the_big_int_evaluation(dumps):
    rnd = random.Random(29)
    for (name, variant), (src, prog, nc, nch) in dumps.items():
        if variant != "2":
            continue
        code, consts, _ = prog.arrays()
        cw = [_word(c) for c in consts]
        for cols, chal, prev in _rows(rnd, nc, len(cw), nch, n=4 if name.startswith("q_") else 8):
            want = E.eval_program(code, cw, chal, prev, lambda c, r: cols[c])
            got = E.concrete(src, cols, cw, chal, prev)
            assert got == want, name


# ---- negative controls: the model is not vacuous ------------------------------------------------------------------------------------
def _edits(src, kind):
    """every source with one line of `kind` removed ("normalize", "reduce") or lowered by one borrow step ("sub", "neg")"""
    lines = src.splitlines()
    out = []
    for i, l in enumerate(lines):
        t = l.strip()
        if kind == "normalize" and re.match(r"v\d+ = Fr29::normalize\(v\d+\);$", t) or \
           kind == "reduce" and re.match(r"v\d+ = Fr29::mul(_cold)?\(v\d+, c_one\);$", t):
            out.append("\n".join(lines[:i] + lines[i + 1:]))
        m = re.search(r"Fr29::%s<(\d)>" % kind, t) if kind in ("sub", "neg") else None
        if m and int(m.group(1)) > 0:
            lower = l.replace("Fr29::%s<%s>" % (kind, m.group(1)), "Fr29::%s<%d>" % (kind, int(m.group(1)) - 1))
            out.append("\n".join(lines[:i] + [lower] + lines[i + 1:]))
    return out


@pytest.mark.parametrize("name,kind", [(n, k) for n, kinds in EP.TIGHT.items() for k in kinds])
def test_model_fails_every_tight_edit(dumps, name, kind):
    """in the families' controls every emitted line of `kind` sits on a limit: the model must refuse each source with one of them removed
    (normalize, reduction) or its borrow lowered by one step (sub, neg)"""
    src = dumps[(name, "2")][0]
    E.worst_case(src)
    edited = _edits(src, kind)
    assert edited, "no %s line in %s" % (kind, name)
    for s in edited:
        with pytest.raises(AssertionError):
            E.worst_case(s)


def test_model_refuses_unknown_lines(dumps):
    """a line outside the known shapes is an error, never skipped"""
    src = dumps[("a_five_loads", "2")][0]
    with pytest.raises(AssertionError, match="not a shape"):
        E.worst_case(src.replace("Fr29::add(", "Fr29::dbl(", 1))


# ---- non-canonical constants and challenges are refused at the C ABI ----------------------------------------------------------------
@pytest.mark.parametrize("word", [P, P + 5, (1 << 256) - 1])
def test_non_canonical_constants_and_challenges_are_refused(word):
    """a constant or challenge word in [p, 2^256) is refused by every entry point's validation (here the two host-only ones).  The model
    shows why: five such constants summed reach ~5 x 169 p after the 5-bit load, and the one final conditional subtraction leaves a wrong word"""
    from ezkl_amd import backend as B, lib as L
    w = np.frombuffer(word.to_bytes(32, "little"), np.uint64).copy()
    prog = B.GraphProgram(3, 5)
    v = prog.constant(w)
    for c in (3, 5, 7, 9):
        v = prog.calc("add", v, prog.constant(np.frombuffer(c.to_bytes(32, "little"), np.uint64).copy()))
    for call in (prog.check_compiles, prog.scheduled_code):
        with pytest.raises(L.EzklHipError) as e:
            call(1)
        assert e.value.code == EZKL_ERR_INVALID
    ok = B.GraphProgram(3, 5)
    ok.calc("add", ok.challenge(0), ok.challenge(1))
    ok.scheduled_code(1)
    for bad in ([[0] * 4, w], [w, [0] * 4]):
        with pytest.raises(L.EzklHipError) as e:
            ok.scheduled_code(1, challenges=np.asarray(bad, np.uint64))
        assert e.value.code == EZKL_ERR_INVALID
    ok.scheduled_code(1, challenges=np.asarray([[0] * 4, np.frombuffer((P - 1).to_bytes(32, "little"), np.uint64)], np.uint64))


def test_model_shows_the_non_canonical_constant_failure():
    """what the validation prevents, on the generated source of a five-term add chain of constants: with every constant at 2^256 - 1 the
    value handed to the final conditional subtraction is not below 2p; with canonical words the result is right"""
    from ezkl_amd import backend as B
    prog = B.GraphProgram(3, 5)
    v = prog.constant(np.zeros(4, np.uint64))
    for c in (1, 2, 3, 4):
        v = prog.calc("add", v, prog.constant(np.asarray([c, 0, 0, 0], np.uint64)))
    code, _, _ = prog.arrays()
    chain = prog.generated_source(1)
    with pytest.raises(AssertionError, match="not below 2p"):
        E.concrete(chain, [], [(1 << 256) - 1] * 5, [0], 0)
    assert E.concrete(chain, [], [P - 1] * 5, [0], 0) == E.eval_program(code, [P - 1] * 5, [0], 0, None)
