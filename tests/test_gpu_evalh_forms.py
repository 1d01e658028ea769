"""Programs that overwrite their intermediates (tests/evalh_forms.py) on the device, in all four kernels of the quotient sweep -- the
hiprtc kernel of each generator (EZKL_EVALH_R29 = 2, 1, 0) and the interpreter -- against the C oracle on every row and against the
big-int evaluator of tools/evalh29_model.py (which runs a program in its own order with a dict of values).  The radix-2^32 generator and
the interpreter (allocate_slots' registers and spills) have no host model: this file is the only check of their values on such programs.
Every jit-mode call must have run exactly one compiled kernel and every interpreter call none (jit_stats): a silent fallback fails.
The host-side passes are checked on the same programs in tests/test_evalh_forms_cpu.py."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
import evalh_forms as F
from evalh_forms import _draw, _ints, _words
import test_gpu_evalh_bounds as TB
from oracle import binding as ob

sys.path.insert(0, os.path.join(ROOT, "tools"))
import evalh29_model as E  # noqa: E402

pytestmark = pytest.mark.gpu
P = E.P
MODES = TB.MODES


def _engine(monkeypatch, tmp_path, mode, r29):
    monkeypatch.setenv("EZKL_EVALH_MODE", mode)
    monkeypatch.setenv("EZKL_EVALH_R29", r29)
    monkeypatch.setenv("EZKL_HIP_CACHE_DIR", str(tmp_path))       # no code object of another build can stand in for this one


def _form(B, name, k=F.K, ext_k=F.EXT_K):
    return {n: (p, nc, nch) for n, p, nc, nch in F.forms(B, k, ext_k)}[name]


def _seed(name):
    return sum(map(ord, name))


@pytest.mark.parametrize("mode,r29", MODES)
@pytest.mark.parametrize("name", F.FORM_NAMES)
def test_every_form_in_every_engine(hip, name, mode, r29, monkeypatch, tmp_path):
    """k = 3, ext_k = 5: three datasets (mixed edges, all p - 1, all 0), every one of the 32 rows (rows 0 and 31, where rotations wrap,
    among them) against the oracle and against the big-int evaluation"""
    from ezkl_amd import backend as B
    _engine(monkeypatch, tmp_path, mode, r29)
    prog, nc, nch = _form(B, name)
    TB._check(B, prog, mode, nc, nch, np.random.default_rng(_seed(name)))


@pytest.mark.parametrize("mode,r29", MODES)
@pytest.mark.parametrize("name", ["ring_9", "ring_10", "ring_40"])
def test_rings_past_one_workgroup(hip, name, mode, r29, monkeypatch, tmp_path):
    """k = 9, ext_k = 11: 2048 rows, the whole output against the oracle and 64 sampled rows against the big-int evaluation"""
    from ezkl_amd import backend as B
    _engine(monkeypatch, tmp_path, mode, r29)
    prog, nc, nch = _form(B, name, 9, 11)
    TB._check(B, prog, mode, nc, nch, np.random.default_rng(_seed(name) + 9))


@pytest.mark.parametrize("mode,r29", [("interp", "2"), ("jit", "2")])
@pytest.mark.parametrize("name", ["ring_10", "ring_40"])
def test_spills_while_a_lane_walks_several_rows(hip, name, mode, r29, monkeypatch, tmp_path):
    """ring_40 (and ring_10: exactly one spilled slot) on 2^17 rows with EZKL_EVALH_TMUL=1: at most 256 x 256 lanes (an MI355X has 256 CUs), so every lane runs its loop at least
    twice.  The interpreter's spill area is [slot][T] + tid: a lane meets the slots of its previous row again.  As scheduled ring_40
    re-acquires spilled slots many times and puts two Horner steps on never-written indices into spilled slots
    (tests/test_evalh_forms_cpu.py pins both): neither may read what the previous row left there"""
    from ezkl_amd import backend as B
    _engine(monkeypatch, tmp_path, mode, r29)
    monkeypatch.setenv("EZKL_EVALH_TMUL", "1")
    prog, nc, nch = _form(B, name, 15, 17)
    code, consts, rots = prog.arrays()
    cw = _ints(consts)
    ne, step, T = 1 << 17, 4, 256 * 256
    rng = np.random.default_rng(17)
    rows = sorted({0, 1, T - 1, T, ne - 1} | {int(x) for x in rng.integers(0, ne, 40)})
    for cols, chal, prev in TB._datasets(rng, ne, nc, nch):
        got = TB._run(B, prog, mode, cols, chal, prev)
        want = ob.eval_program(code, prog.n_intermediates, consts, rots, [_words(c) for c in cols], _words(chal), prog.k, prog.ext_k,
                               previous=_words(prev))
        assert (got == want).all(), "device differs from the oracle"
        gi = _ints(got[rows])
        for j, r in enumerate(rows):
            read = lambda c, ro, r=r: cols[c][(r + int(rots[ro]) * step) % ne]      # noqa: E731
            assert gi[j] == E.eval_program(code, cw, chal, prev[r], read), "row %d differs from the big-int evaluation" % r


@pytest.mark.parametrize("mode,r29", MODES)
def test_reads_of_unwritten_intermediates_are_refused(hip, mode, r29, monkeypatch, tmp_path):
    """EZKL_ERR_INVALID, the output untouched and nothing compiled or launched; the same buffer then takes a valid form"""
    from ezkl_amd import backend as B
    _engine(monkeypatch, tmp_path, mode, r29)
    rng = np.random.default_rng(3)
    ne = 1 << F.EXT_K
    cols, chal, prev = TB._datasets(rng, ne, F.N_COLUMNS, F.N_CHALLENGES)[0]
    dcols = [B.DeviceBuffer.from_numpy(_words(c)) for c in cols]
    dout = B.DeviceBuffer.from_numpy(_words(prev))
    before = TB._jit_total(B)
    for name, prog, nc, nch, _ in F.refused(B):
        with pytest.raises(hip.EzklHipError) as e:
            prog.evaluate_h([d.ptr for d in dcols], _words(chal), dout.ptr)
        assert e.value.code == -3, name                               # EZKL_ERR_INVALID
        assert TB._jit_total(B) == before, name
        assert dout.to_numpy(shape=(ne, 4)).tobytes() == _words(prev).tobytes(), name
    prog, nc, nch = _form(B, "ring_9")
    prog.evaluate_h([d.ptr for d in dcols], _words(chal), dout.ptr)
    assert TB._jit_total(B) - before == (1 if mode == "jit" else 0)
    code, consts, rots = prog.arrays()
    want = ob.eval_program(code, prog.n_intermediates, consts, rots, [_words(c) for c in cols], _words(chal), prog.k, prog.ext_k,
                           previous=_words(prev))
    assert (dout.to_numpy(shape=(ne, 4)) == want).all()
    for d in dcols + [dout]:
        d.free()


# ---- the check kernel on a slot written three times -------------------------------------------------------------------------------
def _check_case(B, k, lo, hi, planted, rng):
    """both programs of evalh_forms.check_programs over rows [lo, hi): column A non-zero on every row, column Z non-zero on `planted`"""
    n = 1 << k
    a = [w or 1 for w in _draw(rng, n)]
    z = [0] * n
    for r, w in zip(planted, [1, P - 1] + [w or 2 for w in _draw(rng, len(planted))]):
        z[r] = w
    da, dz = B.DeviceBuffer.from_numpy(_words(a)), B.DeviceBuffer.from_numpy(_words(z))
    for name, prog, slot in F.check_programs(B, k):
        code, _, _ = prog.arrays()
        assert sum(int(ins[1]) == slot for ins in code) == 3
        last = max(i for i, ins in enumerate(code) if int(ins[1]) == slot)
        first = min(i for i, ins in enumerate(code) if int(ins[1]) == slot)
        val = lambda upto, r: E.eval_program(code[:upto + 1], [], [], 0, lambda c, ro: (a, z)[c][r])      # noqa: E731
        assert all((val(first, r) != 0) == (name == "last_zero") for r in range(n))         # the early version: everywhere, or nowhere
        want = {(1, slot, 0, r) for r in range(lo, hi) if val(last, r) != 0}
        assert want == {(1, slot, 0, r) for r in planted if lo <= r < hi} and len(want) >= 4
        before = TB._jit_total(B)
        records, cnt = prog.check_rows([da.ptr, dz.ptr], np.zeros((0, 4), np.uint64), [slot], lo, hi, cap=n)
        assert TB._jit_total(B) - before == 1
        assert {tuple(int(x) for x in r) for r in records} == want and len(records) == int(cnt[0]) == len(want), name
        cap = len(want) - 2                                                                  # fewer records than failures
        records, cnt = prog.check_rows([da.ptr, dz.ptr], np.zeros((0, 4), np.uint64), [slot], lo, hi, cap=cap)
        got = {tuple(int(x) for x in r) for r in records}
        assert TB._jit_total(B) - before == 2
        assert int(cnt[0]) == len(want) and len(records) == len(got) == cap and got <= want, name
    da.free()
    dz.free()


@pytest.mark.parametrize("r29", ["2", "1"])
def test_check_kernel_reports_the_last_version_of_a_reused_index(hip, r29, monkeypatch, tmp_path):
    """the listed slot is written three times; only its last version decides.  [0, 64) at k = 6: one wave, rows 0 and 63 planted.
    [5, 203) at k = 8: lanes 198 .. 255 never enter the loop while their wave still ballots; planted on both sides of the wave
    boundaries (lanes 63 | 64 are rows 68 | 69), at both ends of the range, and just outside it"""
    from ezkl_amd import backend as B
    _engine(monkeypatch, tmp_path, "jit", r29)
    rng = np.random.default_rng(11)
    _check_case(B, 6, 0, 64, [0, 63, 31, 32, 17], rng)
    _check_case(B, 8, 5, 203, [0, 4, 5, 68, 69, 132, 133, 196, 197, 202, 203, 255], rng)
