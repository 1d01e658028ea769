"""Programs that overwrite their intermediates (tests/evalh_forms.py) through every host-side pass of the quotient sweep
(ezkl_amd/csrc/evalh.hip): schedule_program, allocate_slots' refusals, the two radix-2^29 generators and the check-kernel form, and the
C oracle.  The reference is tools/evalh29_model.eval_program: a big-int evaluator that runs a program in its own order with a dict of
values, and shares nothing with the passes under test.  Host only, no GPU.

What the integer model covers: the source of EZKL_EVALH_R29 = 2 and 1 (sweep and check kernel), worst case and concrete rows.  The
radix-2^32 generator (EZKL_EVALH_R29 = 0) has no integer model: here it is only compiled; its VALUE, and the interpreter's (the slots of
allocate_slots), are checked on the device alone (tests/test_gpu_evalh_forms.py)."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
import evalh_forms as F
from evalh_forms import _draw, _ints, _words
from oracle import binding as ob

sys.path.insert(0, os.path.join(ROOT, "tools"))
import evalh29_model as E  # noqa: E402

P = E.P
EZKL_ERR_INVALID = -3            # include/ezkl_hip.h
N_ROWS = 16


@pytest.fixture(scope="module")
def forms():
    from ezkl_amd import backend as B
    return {n: (p, nc, nch) for n, p, nc, nch in F.forms(B)}


@pytest.fixture(scope="module")
def refused():
    from ezkl_amd import backend as B
    return {n: (p, nc, nch, v) for n, p, nc, nch, v in F.refused(B, 3, 3)}     # k == ext_k: the check kernel takes them too


def _rows(name, n=N_ROWS):
    """n rows of the _draw mix: (one word per column, whatever the rotation; challenges; previous)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    return [(_draw(rng, F.N_COLUMNS), _draw(rng, F.N_CHALLENGES), _draw(rng, 1)[0]) for _ in range(n)]


def _eval(code, cw, rows):
    return [E.eval_program(code, cw, chal, prev, lambda c, r, cols=cols: cols[c]) for cols, chal, prev in rows]


def _key(code):
    return sorted(tuple(int(x) for x in ins) for ins in code)


def test_the_name_lists_are_the_builders(forms, refused):
    """the parametrized cases run by name: a form that forms() builds and the list lacks would never run"""
    from ezkl_amd import backend as B
    assert [n for n, *_ in F.forms(B)] == F.FORM_NAMES and [n for n, *_ in F.refused(B)] == F.REFUSED_NAMES
    assert set(F.HAZARD_FORMS) == {n for n in F.FORM_NAMES if n.startswith("ring_")} | {"self_update"}


def test_the_operands_cover_what_they_claim(forms):
    """the non-tiny forms together read every (column, rotation -2 .. 2), every challenge, every CONST_WORDS entry and `previous`, each
    as operand 0 and as operand 1; self-updating instructions and Horner steps read `previous` too"""
    from evalh_programs import CONST_WORDS
    seen = {0: set(), 1: set()}
    prev_self, prev_horner = False, False
    for name, (prog, _, _) in forms.items():
        if name.startswith("tiny_"):
            continue
        code, consts, rots = prog.arrays()
        cw = _ints(consts)
        for ins in code.tolist():
            for q in range(1 if ins[0] in F.UNARY else 2):
                kind, idx, ro = ins[2 + 3 * q:5 + 3 * q]
                what = {F.CONST: ("const", cw[idx] if kind == F.CONST else 0), F.COLUMN: ("col", idx, int(rots[ro]) if kind == F.COLUMN else 0),
                        F.CHALLENGE: ("chal", idx), F.PREVIOUS: ("prev",), F.INTERMEDIATE: ("int",)}[kind]
                seen[q].add(what)
            kinds = [ins[2 + 3 * q] for q in range(1 if ins[0] in F.UNARY else 2)]
            if F.PREVIOUS in kinds:
                prev_self |= ins[0] != F.HORNER and ins[1] in F.reads(ins)
                prev_horner |= ins[0] == F.HORNER
    want = {("col", c, r) for c in range(F.N_COLUMNS) for r in range(-2, 3)} | {("chal", c) for c in range(F.N_CHALLENGES)} | \
        {("const", w) for w in CONST_WORDS} | {("prev",), ("int",)}
    assert want <= seen[0] and want <= seen[1]
    assert prev_self and prev_horner


def test_the_rings_take_the_slots_they_claim(forms):
    """what each ring exercises in allocate_slots, in the order the library executes it (evalh_forms.slot_plan): ring_3 stays in the
    interpreter's 8 registers, ring_8 and ring_9 -- on both sides of them by index count -- still fit, ring_10 needs exactly one spilled
    slot and takes it more than once, ring_40 spills several, re-acquires them, and puts both Horner steps on never-written indices
    into spilled slots (the row loop must not read what the lane's previous row left there)"""
    plan = {n: F.slot_plan(forms[n][0].scheduled_code(forms[n][1])) for n in F.FORM_NAMES if n.startswith("ring_")}
    assert plan["ring_3"][0] <= 8 and plan["ring_8"][0] <= 8 and plan["ring_9"][0] == 8
    assert plan["ring_10"][0] == 9 and plan["ring_10"][2] >= 2
    used, fresh, again = plan["ring_40"]
    assert used >= 12 and again >= 10 and len(fresh) == 2 and min(fresh) >= 8
    # as written (EZKL_EVALH_NO_SCHEDULE) ring_8 and ring_9 cross the boundary too
    assert F.slot_plan(forms["ring_8"][0].arrays()[0])[0] == 9 and F.slot_plan(forms["ring_9"][0].arrays()[0])[0] == 10


def test_oracle_on_a_program_without_constants():
    """a unary instruction has one operand: its second triple (calc leaves it at constant 0) is not read, here with no constant at all"""
    from ezkl_amd import backend as B
    prog = B.GraphProgram(3, 5)
    prog.calc("negate", prog.calc("store", prog.column(0, -1)))
    code, consts, rots = prog.arrays()
    assert consts.shape[0] == 0
    rng = np.random.default_rng(5)
    col, prev = _draw(rng, 32), _draw(rng, 32)
    got = _ints(ob.eval_program(code, prog.n_intermediates, consts, rots, [_words(col)], np.zeros((0, 4), np.uint64), 3, 5, previous=_words(prev)))
    assert got == [E.eval_program(code, [], [], prev[r], lambda c, ro, r=r: col[(r + int(rots[ro]) * 4) % 32]) for r in range(32)]


@pytest.mark.parametrize("name", F.FORM_NAMES)
def test_schedule_is_a_permutation_with_the_same_value(forms, name):
    prog, nc, _ = forms[name]
    code, consts, _ = prog.arrays()
    sched = prog.scheduled_code(nc)
    assert _key(sched) == _key(code), "the scheduled code is not a permutation of the program"
    assert (sched[-1] == code[-1]).all(), "the last instruction (its target is the result) moved"
    rows = _rows(name)
    assert _eval(sched, _ints(consts), rows) == _eval(code, _ints(consts), rows)


@pytest.mark.parametrize("name", F.FORM_NAMES)
def test_oracle_equals_the_big_int_evaluation(forms, name):
    """the C oracle is the whole-output reference on the device: every row of the 32-row domain, rotations wrapping, three datasets"""
    prog, nc, nch = forms[name]
    code, consts, rots = prog.arrays()
    cw = _ints(consts)
    ne, step = 1 << prog.ext_k, 1 << (prog.ext_k - prog.k)
    rng = np.random.default_rng(sum(map(ord, name)) + 1)
    mixed = ([_draw(rng, ne) for _ in range(nc)], _draw(rng, nch), _draw(rng, ne))
    for cols, chal, prev in (mixed, ([[P - 1] * ne] * nc, [P - 1] * nch, [P - 1] * ne), ([[0] * ne] * nc, _draw(rng, nch), [0] * ne)):
        got = _ints(ob.eval_program(code, prog.n_intermediates, consts, rots, [_words(c) for c in cols], _words(chal), prog.k, prog.ext_k,
                                    previous=_words(prev)))
        for r in range(ne):
            read = lambda c, ro, r=r: cols[c][(r + int(rots[ro]) * step) % ne]      # noqa: E731
            assert got[r] == E.eval_program(code, cw, chal, prev[r], read), "row %d" % r


@pytest.mark.parametrize("schedule", ["scheduled", "as_written"])
@pytest.mark.parametrize("variant", ["2", "1"])
@pytest.mark.parametrize("name", F.FORM_NAMES)
def test_generated_source_holds_its_bounds_and_its_value(forms, name, variant, schedule, monkeypatch):
    """as_written (EZKL_EVALH_NO_SCHEDULE=1) takes the scheduler out: a failure there is the generator's, one in `scheduled` alone the
    scheduler's"""
    prog, nc, _ = forms[name]
    monkeypatch.setenv("EZKL_EVALH_R29", variant)
    if schedule == "as_written":
        monkeypatch.setenv("EZKL_EVALH_NO_SCHEDULE", "1")
    src = prog.generated_source(nc)
    E.worst_case(src)
    code, consts, _ = prog.arrays()
    cw = _ints(consts)
    for cols, chal, prev in _rows(name):
        assert E.concrete(src, cols, cw, chal, prev) == E.eval_program(code, cw, chal, prev, lambda c, r: cols[c])


@pytest.mark.parametrize("variant", ["2", "1", "0"])
@pytest.mark.parametrize("name", F.FORM_NAMES)
def test_every_generator_compiles(forms, name, variant, monkeypatch):
    """hiprtc takes the source of all three generators.  For EZKL_EVALH_R29=0 (radix 2^32) this is all the host can say: it has no integer
    model, its value is checked on the device only"""
    prog, nc, _ = forms[name]
    monkeypatch.setenv("EZKL_EVALH_R29", variant)
    prog.check_compiles(nc)


@pytest.mark.parametrize("variant", ["2", "1"])
def test_check_kernel_tests_the_last_version_of_a_reused_index(variant, monkeypatch):
    from ezkl_amd import backend as B
    monkeypatch.setenv("EZKL_EVALH_R29", variant)
    rng = np.random.default_rng(7)
    for name, prog, slot in F.check_programs(B, 4):
        code, consts, _ = prog.arrays()
        assert sum(int(ins[1]) == slot for ins in code) == 3
        last = max(i for i, ins in enumerate(code) if int(ins[1]) == slot)
        first = min(i for i, ins in enumerate(code) if int(ins[1]) == slot)
        src = prog.check_source(2, [slot])
        E.worst_case(src)
        for a in [w for w in _draw(rng, 12) if w][:6] + [1, P - 1]:
            for z in (0, 1, P - 1, _draw(rng, 1)[0]):
                got = E.concrete_checks(src, [a, z], [], [])
                want = E.eval_program(code[:last + 1], [], [], 0, lambda c, r: [a, z][c])
                early = E.eval_program(code[:first + 1], [], [], 0, lambda c, r: [a, z][c])
                assert got == {slot: want}
                assert (want != 0) == (z != 0) and (early != 0) == (name == "last_zero")     # the programs are what they claim
        # in the rows with z == 0 of last_zero an earlier version is non-zero and the last is zero; in the rows with z != 0 of
        # last_nonzero it is the other way round


@pytest.mark.parametrize("name", F.REFUSED_NAMES)
def test_reads_of_unwritten_intermediates_are_refused(refused, name, monkeypatch):
    from ezkl_amd import lib as L
    prog, nc, _, by_validation = refused[name]
    code, consts, _ = prog.arrays()
    with pytest.raises(KeyError):                                  # the reference refuses it too
        E.eval_program(code, _ints(consts), [1] * F.N_CHALLENGES, 1, lambda c, r: 1)
    written = sorted({int(ins[1]) for ins in code})
    calls = [lambda: prog.generated_source(nc), lambda: prog.check_compiles(nc), lambda: prog.check_source(nc, written[:1])]
    if by_validation:
        calls.append(lambda: prog.scheduled_code(nc))
    else:                                                          # the operand check alone cannot tell: the order comes back, and is still
        sched = prog.scheduled_code(nc)                            # a program the reference refuses
        assert _key(sched) == _key(code)
        with pytest.raises(KeyError):
            E.eval_program(sched, _ints(consts), [1] * F.N_CHALLENGES, 1, lambda c, r: 1)
    for variant in ("2", "1", "0"):
        monkeypatch.setenv("EZKL_EVALH_R29", variant)
        for no_schedule in (False, True):
            if no_schedule:
                monkeypatch.setenv("EZKL_EVALH_NO_SCHEDULE", "1")
            else:
                monkeypatch.delenv("EZKL_EVALH_NO_SCHEDULE", raising=False)
            for call in calls:
                with pytest.raises(L.EzklHipError) as e:
                    call()
                assert e.value.code == EZKL_ERR_INVALID


@pytest.mark.parametrize("name", F.HAZARD_FORMS)
def test_the_forms_would_catch_a_dropped_edge(forms, name):
    """each of these forms holds adjacent pairs tied by a write-after-read edge alone, and by a write-after-write edge alone; the program
    with such a pair swapped -- what a scheduler without that edge may emit -- has another value on the test rows.  Asserted for EVERY
    pair whose value matters, not for one that happens to differ.  A pair counts when the swap changes the value its instruction writes
    (x * x read before or after x = -x is the same value: no hazard in value) and nudging that value (adding a constant right behind
    the instruction) moves the result on these rows.  Being read on the way to the result is not enough -- with three indices
    x2 - (x2 - c) and its like cancel values out again"""
    prog, _, _ = forms[name]
    code, consts, _ = prog.arrays()
    cw = _ints(consts)
    one = cw.index(1)                                              # CONST_WORDS holds the word 1: any non-zero constant will do
    rows = _rows(name)
    want = _eval(code, cw, rows)
    for kind, orders in zip(("WAR", "WAW"), F.hazard_orders(code)):
        orders = [o for j, at, o in orders if _eval(o[:at + 1], cw, rows) != _eval(code[:j + 1], cw, rows)
                  and _eval(F.nudged(code, j, one), cw, rows) != want]
        assert orders, "no %s pair that matters in %s: the form is wrong" % (kind, name)
        for order in orders:
            assert _key(order) == _key(code)
            assert _eval(order, cw, rows) != want, "%s: a violated %s edge does not change the value" % (name, kind)
