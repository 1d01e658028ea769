"""The mock prover's host side (`ezkl mock`: ezkl_prover_mock, ezkl_hip_eval_check_* / _lookup_missing_rows_dev / _copy_check_dev): the
C ABI refuses malformed calls before it touches a device, reports a missing GPU, and the gate-check kernel the sweep JIT generates passes
the worst-case limb model of tools/evalh29_model.py.  The quotient sweep's own source is pinned: the check mode did not change it.  No GPU
needed; the kernels run in tests/test_gpu_mock.py."""
import ctypes as C
import hashlib
import os
import random
import sys

import numpy as np
import pytest

from conftest import ROOT
import evalh_programs as EP

sys.path.insert(0, os.path.join(ROOT, "tools"))
import evalh29_model as E  # noqa: E402

EZKL_ERR_NO_DEVICE, EZKL_ERR_INVALID = -1, -3          # include/ezkl_hip.h

# sha256 of ezkl_hip_eval_h_source for the quotient programs of tests/evalh_programs.circuit_programs, per EZKL_EVALH_R29, taken on the
# tree before the check mode was added: the sweep kernels (and their on-disk cache entries) are unchanged
PINNED = {
    ("2", "q_fixture_k6"): "ff228f18987b3ae13a1c482c96e1f0ff83ca33fca43c2d927063e5cc4942b91f",
    ("2", "q_mlp"): "6dc261d3dee4150524e87ba767e8c3ab00baf38fc01acb3b0fb66f62f669c6ab",
    ("2", "q_surrogate"): "fe9379a5613eddc4db7f6956652f2acbfd67c7466130164bd833c2f2754ccf6d",
    ("1", "q_fixture_k6"): "11f9f429a2a9539d30f5c5273e9293ee8e4884a47928da5c78bb670570d3e7d9",
    ("1", "q_mlp"): "4d230a300825cdc9dc24e56c9e701bda21f0dc55aee038cee01896651be91388",
    ("1", "q_surrogate"): "62aa473a94cf648bda57a5e1707384f3770dbe9f37ac6e78164c678391db42ee",
    ("0", "q_fixture_k6"): "8509bc75f30aaa0e7a8d5c082b2ce1575bf5179f8338495b0281b921013c17b8",
    ("0", "q_mlp"): "8e1a8ee744e26c25c6387f80572c930e487e4decf07eaac16e610b2b4e71a625",
    ("0", "q_surrogate"): "22ad7efdf2c81c58063fe8220beea389197da470622890eaade30779ef0e788e",
}


def gate_check_program(cs):
    """the check program ezkl_prover_mock builds: every gate lowered once (shared subexpressions shared) and STORE'd to a slot of its own,
    k == ext_k.  -> (GraphProgram, slots, number of columns, number of challenges)"""
    from ezkl_amd import backend as B, plonk as P
    prog = B.GraphProgram(cs.k, cs.k)
    index = {}

    def col_index(kind, c):
        if kind == "chal":
            return prog.challenge(c)
        return index.setdefault((kind, c), len(index))
    memo, slots = {}, []
    for g in cs.gates:
        slots.append(prog.calc("store", P.lower(g, prog, col_index, memo))[1])
    return prog, slots, len(index), max(1, cs.n_challenges)


def _circuits():
    import fixture_k6 as FX
    from ezkl_amd import ezkl_layout as EL
    sur = EL.TransformerSurrogateCircuit(10, blocks=2, d=4, einsum_len=3, decomp_base=16, lookup_max=(1 << 10) // 16)
    return [("fixture_k6", FX.load()["cs"]), ("surrogate", sur.build(tiles=1)["cs"])]


@pytest.fixture(scope="module")
def check_programs():
    return [(name,) + gate_check_program(cs) for name, cs in _circuits()]


def test_both_libraries_export_the_mock_symbols():
    from ezkl_amd import lib, native
    for s in ("ezkl_hip_eval_check_dev", "ezkl_hip_eval_check_source", "ezkl_hip_lookup_missing_rows_dev", "ezkl_hip_copy_check_dev"):
        assert s in lib.SYMBOLS and hasattr(lib.load(), s)
    assert "ezkl_prover_mock" in native.SYMBOLS and hasattr(native.load(), "ezkl_prover_mock")
    from ezkl_amd import execute
    assert callable(execute.mock) and issubclass(execute.MockError, ValueError)


@pytest.mark.parametrize("variant", ["2", "1", "0"])
def test_sweep_source_is_byte_identical(variant, monkeypatch):
    monkeypatch.setenv("EZKL_EVALH_R29", variant)
    for name, prog, nc, _ in EP.circuit_programs():
        assert hashlib.sha256(prog.generated_source(nc).encode()).hexdigest() == PINNED[(variant, name)], name


@pytest.mark.parametrize("variant", ["2", "1"])
def test_check_source_passes_the_worst_case_model(check_programs, variant, monkeypatch):
    monkeypatch.setenv("EZKL_EVALH_R29", variant)
    for name, prog, slots, nc, nch in check_programs:
        src = prog.check_source(nc, slots)
        assert "void evalh_check(" in src and "evalh_jit" not in src and "st_fe(" not in src
        assert src.count("ezkl_report(") == len(slots) + 1                      # one report per gate, plus the helper's definition
        E.worst_case(src)


def test_check_source_values_are_the_gates(check_programs):
    """concrete mode: on random rows the value each report tests is the big-int value of its gate"""
    rnd = random.Random(7)
    for name, prog, slots, nc, nch in check_programs:
        src = prog.check_source(nc, slots)
        code, consts, _ = prog.arrays()
        cw = [int.from_bytes(np.ascontiguousarray(c, np.uint64).tobytes(), "little") for c in consts]
        writer = {int(ins[1]): i for i, ins in enumerate(code.tolist())}
        for _ in range(3):
            cols = [rnd.randrange(E.P) for _ in range(nc)]
            chal = [rnd.randrange(E.P) for _ in range(nch)]
            got = E.concrete_checks(src, cols, cw, chal)
            assert sorted(got) == sorted(slots)
            for j in slots:
                want = E.eval_program(code[:writer[j] + 1].tolist(), cw, chal, 0, lambda c, r: cols[c])
                assert got[j] == want, (name, j)


def test_model_refuses_an_altered_report_line(check_programs):
    name, prog, slots, nc, nch = check_programs[0]
    src = prog.check_source(nc, slots)
    bad = src.replace("ezkl_report(", "ezkl_reportx(", 2)
    with pytest.raises(AssertionError):
        E.worst_case(bad)


def test_check_mode_refuses_bad_calls(check_programs, monkeypatch):
    from ezkl_amd import backend as B, lib
    L = lib.load()
    name, prog, slots, nc, nch = check_programs[0]
    pr, keep = prog._host_program(nc, None)
    sl = (C.c_uint32 * len(slots))(*slots)
    n = C.c_size_t(0)
    assert L.ezkl_hip_eval_check_source(None, sl, C.c_uint32(len(slots)), None, C.c_size_t(0), C.byref(n)) == EZKL_ERR_INVALID
    assert L.ezkl_hip_eval_check_source(C.byref(pr), None, C.c_uint32(len(slots)), None, C.c_size_t(0), C.byref(n)) == EZKL_ERR_INVALID
    assert L.ezkl_hip_eval_check_source(C.byref(pr), sl, C.c_uint32(0), None, C.c_size_t(0), C.byref(n)) == EZKL_ERR_INVALID
    for bad in ([prog.n_intermediates], [slots[0], slots[0]]):                   # out of range, listed twice
        b = (C.c_uint32 * len(bad))(*bad)
        assert L.ezkl_hip_eval_check_source(C.byref(pr), b, C.c_uint32(len(bad)), None, C.c_size_t(0), C.byref(n)) == EZKL_ERR_INVALID
    ext = B.GraphProgram(prog.k, prog.k + 1)                                     # the check runs on the 2^k rows: ext_k must equal k
    ext.code, ext.constants, ext.rotations, ext.n_intermediates = prog.code, prog.constants, prog.rotations, prog.n_intermediates
    pe, keep2 = ext._host_program(nc, None)
    assert L.ezkl_hip_eval_check_source(C.byref(pe), sl, C.c_uint32(len(slots)), None, C.c_size_t(0), C.byref(n)) == EZKL_ERR_INVALID
    monkeypatch.setenv("EZKL_EVALH_R29", "0")                                    # radix-2^32 generator: no check form
    assert L.ezkl_hip_eval_check_source(C.byref(pr), sl, C.c_uint32(len(slots)), None, C.c_size_t(0), C.byref(n)) == EZKL_ERR_INVALID
    monkeypatch.delenv("EZKL_EVALH_R29")
    cnt = C.c_void_p(8)                                                          # never dereferenced: every call below is refused first
    assert L.ezkl_hip_eval_check_dev(C.byref(pr), sl, C.c_uint32(len(slots)), 0, 8, None, C.c_uint32(4), cnt, None) == EZKL_ERR_INVALID
    assert L.ezkl_hip_eval_check_dev(C.byref(pr), sl, C.c_uint32(len(slots)), 0, 8, None, C.c_uint32(0), None, None) == EZKL_ERR_INVALID
    tabs = (C.c_void_p * 1)(16)
    assert L.ezkl_hip_lookup_missing_rows_dev(None, None, 0, None, 1, 64, 32, None, 0, cnt, None) == EZKL_ERR_INVALID
    assert L.ezkl_hip_lookup_missing_rows_dev(None, None, 0, tabs, 0, 64, 32, None, 0, cnt, None) == EZKL_ERR_INVALID
    assert L.ezkl_hip_lookup_missing_rows_dev(None, None, 0, tabs, 1, 64, 32, None, 4, cnt, None) == EZKL_ERR_INVALID
    assert L.ezkl_hip_lookup_missing_rows_dev(None, None, 1, tabs, 1, 64, 32, None, 0, cnt, None) == EZKL_ERR_INVALID
    cols = (C.c_void_p * 2)(16, None)
    assert L.ezkl_hip_copy_check_dev(cols, 2, C.c_void_p(16), 6, None, 0, cnt, None) == EZKL_ERR_INVALID      # a null column
    assert L.ezkl_hip_copy_check_dev(cols, 1, None, 6, None, 0, cnt, None) == EZKL_ERR_INVALID                # no successor map
    assert L.ezkl_hip_copy_check_dev(cols, 1, C.c_void_p(16), 6, None, 4, cnt, None) == EZKL_ERR_INVALID      # cap without records
    assert L.ezkl_hip_copy_check_dev(cols, 1, C.c_void_p(16), 29, None, 0, cnt, None) == EZKL_ERR_INVALID     # log_n out of range


def _mock_args(cs, fixed, copies, adv, inst):
    from ezkl_amd import native as NV, plonk as P
    keep = [np.ascontiguousarray(np.stack([P.to_mont(v) for v in col]), np.uint64) for col in fixed]
    fx = NV._ptr_array(keep)
    av = [np.ascontiguousarray(np.stack([P.to_mont(v) for v in col]), np.uint64) for col in adv]
    keep += av
    ins = [np.ascontiguousarray(np.stack([P.to_mont(v) for v in col]) if len(col) else np.zeros((0, 4), np.uint64), np.uint64) for col in inst]
    keep += ins
    lens = (C.c_uint32 * max(1, len(ins)))(*[a.shape[0] for a in ins])
    cp = NV._copies_array(copies)
    return fx, cp, NV._ptr_array(av), NV._ptr_array(ins), lens, keep


def _lookup_fixture():
    """the k = 6 lookup circuit of tests/test_plonk.py: (cs, fixed, copies, advice), columns as lists of ints"""
    import test_plonk as TP
    from ezkl_amd import plonk as P
    cs = TP.lookup_circuit(6)
    adv, fixed, copies = TP.lookup_witness(cs, 4)
    ints = lambda cols: [[P.from_mont(w) for w in np.asarray(c, np.uint64).reshape(-1, 4)] for c in cols]
    return cs, ints(fixed), [((0, 1), (1, 1))] + list(copies), ints(adv)


def test_prover_mock_refuses_malformed_calls():
    from ezkl_amd import native as NV, plonk as P
    cs, fixed, copies, adv = _lookup_fixture()
    circ = NV.NativeCircuit(cs)
    fx, cp, av, ins, lens, keep = _mock_args(cs, fixed, copies, adv, [[] for _ in range(cs.n_instance)])
    out = (NV.CheckRecord * 4)()
    tot = (C.c_uint64 * 3)()
    n = C.c_size_t(0)
    Lp = NV.load()
    ok = dict(h=circ.h, fx=fx, cp=cp.ctypes.data_as(C.c_void_p), ncp=C.c_size_t(cp.shape[0]), av=av, ins=ins, lens=lens, out=out, cap=C.c_size_t(4), tot=tot, n=C.byref(n))

    def call(**kw):
        a = dict(ok, **kw)
        return Lp.ezkl_prover_mock(a["h"], a["fx"], a["cp"], a["ncp"], a["av"], None, None, a["ins"], a["lens"], C.c_uint64(1), a["out"], a["cap"], a["tot"], a["n"])
    assert call(h=None) == EZKL_ERR_INVALID
    assert call(out=None) == EZKL_ERR_INVALID                                     # cap > 0 and no output array
    assert call(tot=None) == EZKL_ERR_INVALID
    assert call(n=None) == EZKL_ERR_INVALID
    assert call(fx=None) == EZKL_ERR_INVALID
    assert call(av=None) == EZKL_ERR_INVALID                                      # no advice columns and no callback
    assert call(cp=None, ncp=C.c_size_t(1)) == EZKL_ERR_INVALID                   # copies announced, none given
    bad = np.array([[len(cs.perm), 0, 0, 0]], np.uint32)                          # a copy into a column the permutation does not have
    assert call(cp=bad.ctypes.data_as(C.c_void_p), ncp=C.c_size_t(1)) == EZKL_ERR_INVALID
    bad = np.array([[0, cs.n, 0, 0]], np.uint32)                                  # a row past the domain
    assert call(cp=bad.ctypes.data_as(C.c_void_p), ncp=C.c_size_t(1)) == EZKL_ERR_INVALID
    circ.free()


@pytest.mark.skipif(__import__("ezkl_amd.lib", fromlist=["load"]).load().ezkl_hip_device_count() > 0, reason="GPU present")
def test_prover_mock_without_a_device_is_no_device():
    from ezkl_amd import native as NV, plonk as P
    cs, fixed, copies, adv = _lookup_fixture()
    circ = NV.NativeCircuit(cs)
    fx, cp, av, ins, lens, keep = _mock_args(cs, fixed, copies, adv, [[] for _ in range(cs.n_instance)])
    out = (NV.CheckRecord * 4)()
    tot = (C.c_uint64 * 3)()
    n = C.c_size_t(0)
    rc = NV.load().ezkl_prover_mock(circ.h, fx, cp.ctypes.data_as(C.c_void_p), C.c_size_t(cp.shape[0]), av, None, None, ins, lens, C.c_uint64(1), out,
                                    C.c_size_t(4), tot, C.byref(n))
    assert rc == EZKL_ERR_NO_DEVICE
    with pytest.raises(RuntimeError, match="ezkl_prover_mock"):
        NV.mock(cs, [np.stack([P.to_mont(v) for v in c]) for c in fixed], copies, [np.stack([P.to_mont(v) for v in c]) for c in adv],
                instances=[[] for _ in range(cs.n_instance)])
    circ.free()
