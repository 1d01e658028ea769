"""The quotient sweep at the bounds of its arithmetic: the programs of tests/evalh_programs.py (each on one limit of the radix-2^29 code
generator) on the device with extreme words, in all four kernels -- the hiprtc kernel of each generator (EZKL_EVALH_R29 = 2, 1, 0) and the
interpreter -- against the oracle on every row and against the pure-Python big-int evaluator of tools/evalh29_model.py on 64 rows
(rows 0 and ne - 1, where rotations wrap, among them).  Every jit-mode call must have run a compiled kernel (jit_stats).  Also: the
vector kernels on full-range and all-(p - 1) columns, and the refusal of non-canonical constants and challenges."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
import evalh_programs as EP
from evalh_forms import _draw, _ints, _words
from oracle import binding as ob

sys.path.insert(0, os.path.join(ROOT, "tools"))
import evalh29_model as E  # noqa: E402

pytestmark = pytest.mark.gpu
P = E.P
MODES = [("jit", "2"), ("jit", "1"), ("jit", "0"), ("interp", "2")]


def _datasets(rng, ne, ncols, nchal):
    """(columns, challenges, previous) as int lists: per-row mixes; every column and previous at p - 1; every column and previous 0 (each
    subtraction then lands on a + K p exactly)"""
    mixed = ([_draw(rng, ne) for _ in range(ncols)], _draw(rng, nchal), _draw(rng, ne))
    return [mixed,
            ([[P - 1] * ne for _ in range(ncols)], [P - 1] * nchal, [P - 1] * ne),
            ([[0] * ne for _ in range(ncols)], _draw(rng, nchal), [0] * ne)]


def _jit_total(B):
    return sum(B.jit_stats())


def _run(B, prog, mode, cols, chal, prev):
    """one sweep on the device; jit mode must have launched a compiled kernel (exactly one more compiled / loaded / found kernel)"""
    dcols = [B.DeviceBuffer.from_numpy(_words(c)) for c in cols]
    dout = B.DeviceBuffer.from_numpy(_words(prev))
    before = _jit_total(B)
    prog.evaluate_h([d.ptr for d in dcols], _words(chal), dout.ptr)
    ne = len(prev)
    got = dout.to_numpy(shape=(ne, 4))
    assert _jit_total(B) - before == (1 if mode == "jit" else 0), "jit mode did not run a compiled kernel" if mode == "jit" else "interp ran the jit"
    for d in dcols + [dout]:
        d.free()
    return got


def _check(B, prog, mode, ncols, nchal, rng):
    code, consts, rots = prog.arrays()
    cw = _ints(consts)
    ne = 1 << prog.ext_k
    step = 1 << (prog.ext_k - prog.k)
    rows = sorted({0, ne - 1, 1, ne - 2} | {int(x) for x in rng.integers(0, ne, 60)}) if ne > 64 else list(range(ne))
    for cols, chal, prev in _datasets(rng, ne, ncols, nchal):
        got = _run(B, prog, mode, cols, chal, prev)
        want = ob.eval_program(code, prog.n_intermediates, consts, rots, [_words(c) for c in cols], _words(chal), prog.k, prog.ext_k,
                               previous=_words(prev))
        assert (got == want).all(), "device differs from the oracle"
        gi = _ints(got[rows])
        for j, r in enumerate(rows):
            read = lambda c, ro, r=r: cols[c][(r + int(rots[ro]) * step) % ne]      # noqa: E731
            assert gi[j] == E.eval_program(code, cw, chal, prev[r], read), "row %d differs from the big-int evaluation" % r


def _family(name):
    from ezkl_amd import backend as B
    return dict(EP.families(B))[name]


@pytest.mark.parametrize("mode,r29", MODES)
@pytest.mark.parametrize("name", ["a_five_loads", "a_double_to_L6", "a_sum_to_160", "b_sub_neg_bands", "b_sub_reduce", "b_neg_loads",
                                  "b_sub_loads", "c_products", "c_product_reduce", "c_mul_normalize", "c_loose3_squared",
                                  "d_horner", "e_same_operand",
                                  "f_sub_160", "f_sum_152", "f_horner_157"])
def test_families_at_the_bounds(hip, name, mode, r29, monkeypatch, tmp_path):
    from ezkl_amd import backend as B
    monkeypatch.setenv("EZKL_EVALH_MODE", mode)
    monkeypatch.setenv("EZKL_EVALH_R29", r29)
    monkeypatch.setenv("EZKL_HIP_CACHE_DIR", str(tmp_path))       # no stale code object from another build can stand in for this one
    _check(B, _family(name), mode, EP.N_COLUMNS, EP.N_CHALLENGES, np.random.default_rng(sum(map(ord, name))))


@pytest.mark.parametrize("mode,r29", MODES)
def test_row_loop_runs_more_than_once(hip, mode, r29, monkeypatch, tmp_path):
    """2^18 rows; EZKL_EVALH_TMUL=1 launches one workgroup of 256 lanes per CU (256 x 256 on an MI355X), so every lane walks several rows"""
    from ezkl_amd import backend as B
    monkeypatch.setenv("EZKL_EVALH_MODE", mode)
    monkeypatch.setenv("EZKL_EVALH_R29", r29)
    monkeypatch.setenv("EZKL_HIP_CACHE_DIR", str(tmp_path))
    monkeypatch.setenv("EZKL_EVALH_TMUL", "1")
    prog = dict(EP.fam_c(B, k=16, ext_k=18))["c_products"]
    _check(B, prog, mode, EP.N_COLUMNS, EP.N_CHALLENGES, np.random.default_rng(18))


@pytest.mark.parametrize("mode,r29", MODES)
@pytest.mark.parametrize("where", ["constant", "challenge"])
@pytest.mark.parametrize("bad", [P, P + 5, (1 << 256) - 1])
def test_non_canonical_constant_or_challenge_is_refused(hip, where, bad, mode, r29, monkeypatch, tmp_path):
    """a word in [p, 2^256) as one term of a five-term add chain: the generated kernel would add up to ~169 p per such load and hand the
    last conditional subtraction a value far above 2 p (tools/evalh29_model.py shows it on the source), so the call is refused before
    anything runs, and the output is left alone"""
    from ezkl_amd import backend as B
    monkeypatch.setenv("EZKL_EVALH_MODE", mode)
    monkeypatch.setenv("EZKL_EVALH_R29", r29)
    monkeypatch.setenv("EZKL_HIP_CACHE_DIR", str(tmp_path))
    prog = B.GraphProgram(3, 5)
    chal = [3, 5]
    if where == "constant":
        v = prog.constant(_words([bad])[0])
    else:
        v = prog.challenge(1)
        chal[1] = bad
    for c in (7, 11, 13, 17):
        v = prog.calc("add", v, prog.constant(_words([c])[0]))
    v = prog.calc("add", v, prog.challenge(0))
    ne = 32
    col = B.DeviceBuffer.from_numpy(_words([1] * ne))
    prev = _words(range(ne))
    dout = B.DeviceBuffer.from_numpy(prev)
    before = _jit_total(B)
    with pytest.raises(hip.EzklHipError) as e:
        prog.evaluate_h([col.ptr], _words(chal), dout.ptr)
    assert e.value.code == -3                                     # EZKL_ERR_INVALID
    assert _jit_total(B) == before and (dout.to_numpy(shape=(ne, 4)) == prev).all()
    # the same chain with the canonical words p - 1 runs, and is right
    if where == "constant":
        prog.constants[0] = _words([P - 1])[0]
    else:
        chal[1] = P - 1
    prog.evaluate_h([col.ptr], _words(chal), dout.ptr)
    code, consts, rots = prog.arrays()
    want = E.eval_program(code, _ints(consts), chal, 0, None)
    assert set(_ints(dout.to_numpy(shape=(ne, 4)))) == {want}


# ---- the vector kernels on full-range and all-(p - 1) columns ------------------------------------------------------------------------
RINV = pow(1 << 256, -1, P)


def _val(w):
    return w * RINV % P


def _mont(x):
    return x * (1 << 256) % P


@pytest.mark.parametrize("n", [1, 31, 32, 33, (1 << 16) + 3])
@pytest.mark.parametrize("fill", ["full_range", "all_p_minus_1"])
def test_vector_kernels_at_the_bounds(hip, n, fill):
    from ezkl_amd import backend as B
    rng = np.random.default_rng(n + (7 if fill == "full_range" else 0))
    if fill == "full_range":
        a, b = _draw(rng, n), _draw(rng, n)
    else:
        a, b = [P - 1] * n, [P - 1] * n
    aw, bw = _words(a), _words(b)
    x = _draw(rng, 1)[0] if fill == "full_range" else P - 1
    small = n <= 4096
    da, db, do = B.DeviceBuffer.from_numpy(aw), B.DeviceBuffer.from_numpy(bw), B.DeviceBuffer(n * 32)
    for op in ("add", "sub", "mul"):
        B.vec_op(op, da.ptr, db.ptr, do.ptr, n)
        got = do.to_numpy(shape=(n, 4))
        assert (got == ob.vec_op(op, aw, bw)).all(), op
        if small:
            f = {"add": lambda u, v: (u + v) % P, "sub": lambda u, v: (u - v) % P, "mul": lambda u, v: u * v * RINV % P}[op]
            assert _ints(got) == [f(u, v) for u, v in zip(a, b)], op
    # eval_polynomial: Horner over the whole vector
    got = _ints(B.eval_polynomial(da.ptr, n, _words([x])[0]))[0]
    assert got == _ints(ob.eval_poly(aw, _words([x])[0]))[0]
    if small:
        acc, xv = 0, _val(x)
        for w in reversed(a):
            acc = (acc * xv + _val(w)) % P
        assert got == _mont(acc)
    # lincomb of two inputs with full-range coefficients, and accumulated on top
    cf = [x, P - 1]
    B.lincomb([da.ptr, db.ptr], _words(cf), do.ptr, n)
    lc = [(u * _val(cf[0]) + v * _val(cf[1])) % P for u, v in zip(a, b)] if small else None
    got = do.to_numpy(shape=(n, 4))
    assert (got == ob.vec_add(ob.vec_scale(aw, _words([cf[0]])[0]), ob.vec_scale(bw, _words([cf[1]])[0]))).all()
    if small:
        assert _ints(got) == lc
    # kate_division by (X - x)
    B.kate_division(da.ptr, _words([x])[0], do.ptr, n)
    got = do.to_numpy(shape=(n, 4))
    assert (got == ob.kate_div(aw, _words([x])[0])).all()
    if small:
        q, carry, xv = [0] * n, 0, _val(x)
        for i in reversed(range(n)):
            q[i] = _mont(carry)
            carry = (carry * xv + _val(a[i])) % P
        assert _ints(got) == q
    # prefix scans (sum and product, inclusive and exclusive)
    for op in ("add", "mul"):
        for excl in (False, True):
            B.prefix_scan(op, da.ptr, do.ptr, n, exclusive=excl)
            got = do.to_numpy(shape=(n, 4))
            assert (got == ob.prefix_scan(aw, op, exclusive=excl)).all(), (op, excl)
            if small:
                acc, want = (0 if op == "add" else 1), []
                for w in a:
                    nxt = (acc + _val(w)) % P if op == "add" else acc * _val(w) % P
                    want.append(_mont(acc if excl else nxt))
                    acc = nxt
                assert _ints(got) == want, (op, excl)
    # batch inversion (zeros stay zero)
    B.batch_invert(da.ptr, n)
    got = da.to_numpy(shape=(n, 4))
    assert (got == ob.batch_invert(aw)).all()
    if small:
        assert _ints(got) == [_mont(pow(_val(w), -1, P)) if w else 0 for w in a]
    for d in (da, db, do):
        d.free()
