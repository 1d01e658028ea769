"""Witness plans with phases, without a GPU (ezkl_amd/witness_plan.py): the layout of an EinsumMatmulCircuit -- Freivalds' argument, whose
second-phase columns depend on two challenges squeezed after the first-phase commitments -- recorded once from the circuit's own
`sequence` and replayed by `run_plan_host` must reproduce the circuit's per-phase `advice_fn` cell for cell, and the oracle MockProver
must accept the result.  The blob keeps version 1 (the phases live in words that were reserved zeros), the record count does not grow
with the matrix, both validators -- the Python mirror and csrc/witness_plan.hpp through libezkl_prover.so -- refuse a bad phase, challenge,
matmul or rlc record with the same words, and hand-built matmul / rlc plans agree with a direct formula at the value and shape edges."""
import struct

import numpy as np
import pytest

SIZES = [(6, 3), (10, 17)]
ROWS = {(6, 3): (35, 58), (10, 17): (903, 1018)}                  # rows the layout uses, of the usable ones
CHAL = [0x1234567890abcdef1234567890abcdef, 0xfedcba0987654321]
M31 = (1 << 31) - 1


def einsum_case(k, L, seed=1):
    from ezkl_amd import ezkl_layout as EL
    c = EL.EinsumMatmulCircuit(k, L)
    rng = np.random.default_rng(seed)
    a, b = rng.integers(-128, 128, (L, L)), rng.integers(-128, 128, (L, L))
    return c, a, b, [int(v) for v in a.reshape(-1)] + [int(v) for v in b.reshape(-1)]


_RECORDED = {}


def recorded(k, L):
    """(circuit, a, b, inputs, plan): recorded once, shared, never modified"""
    from ezkl_amd import witness_plan as WP
    if (k, L) not in _RECORDED:
        c, a, b, x = einsum_case(k, L)
        _RECORDED[(k, L)] = (c, a, b, x, WP.record_plan(c))
    return _RECORDED[(k, L)]


@pytest.mark.parametrize("k,L", SIZES)
def test_host_interpreter_reproduces_the_einsum_layout_phase_by_phase(k, L):
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    from oracle import mock_prover as MP
    R = EL.R
    c, a, b, x, plan = recorded(k, L)
    cs, fixed, copies, rows = c.keygen_inputs(a, b)
    assert (rows, cs.usable) == ROWS[(k, L)]
    fn = c.advice_fn(a, b, cs.n_advice)
    assert plan.n_advice == cs.n_advice == 6 and plan.n_inputs == 2 * L * L and plan.n_phases == 2 and plan.n_challenges == 2 and len(plan.outputs) == 0
    assert WP.column_phases(plan) == cs.advice_phase
    first = fn(0, [])
    cols, outs = WP.run_plan_host(plan, x, phase=0)
    assert outs == []
    for i, ref in first.items():
        assert cols[i] == ref, "phase 0: advice column %d differs" % i
    assert all(not any(cols[i]) for i in range(6) if cs.advice_phase[i] == 1), "phase 0 alone leaves the second-phase columns zero"
    chal = [v % R for v in CHAL]
    both = {**first, **fn(1, chal)}
    cols, _ = WP.run_plan_host(plan, x, challenges=chal)
    for i in range(6):
        assert cols[i] == both[i], "advice column %d differs" % i
    assert MP.check(cs, cols, fixed, [], copies, challenges=chal) == []
    # other inputs, other challenges: the same plan
    c2, a2, b2, x2 = einsum_case(k, L, seed=5)
    chal2 = [R - 1, 3]
    fn2 = c.advice_fn(a2, b2, cs.n_advice)
    cols2, _ = WP.run_plan_host(plan, x2, challenges=chal2)
    assert cols2 == [{**fn2(0, []), **fn2(1, chal2)}[i] for i in range(6)]
    with pytest.raises(ValueError, match="challenges"):
        WP.run_plan_host(plan, x)


# (k, L) -> (sha256 of the recorded blob, the first 16 hex digits of params_hash), taken on commit 50e40f7
PINS = {(6, 3): ("0e654702bf8063410af28610c93314b9dc9350958cce4c6235f80d2b7612ebc8", "8dfda4fe13ce79f1"),
        (10, 17): ("d7b905c435ba69a10cd0ebe780fd5a71fa8086fe1e54f5c3d82b91bd3e2c8d9d", "60b3fbc27bb4cfae")}


@pytest.mark.parametrize("k,L", SIZES)
def test_einsum_plans_keep_their_bytes(k, L):
    import hashlib
    from ezkl_amd import witness_plan as WP
    c, _, _, _, plan = recorded(k, L)
    assert (plan.n_records, hashlib.sha256(plan.to_bytes()).hexdigest(), WP.params_hash(c).hex()[:16]) == (8,) + PINS[(k, L)]


def test_blob_keeps_version_1_and_the_record_count_does_not_follow_the_matrix():
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    (c3, _, _, _, p3), (c17, _, _, _, p17) = recorded(6, 3), recorded(10, 17)
    for c, plan in ((c3, p3), (c17, p17)):
        blob = plan.to_bytes()
        again = WP.WitnessPlan.from_bytes(blob)
        assert again.to_bytes() == blob and again == plan and (again.n_challenges, again.n_phases) == (2, 2)
        head = struct.unpack_from("<20I", blob)
        assert head[1] == WP.VERSION == 1 and (head[14], head[15]) == (2, 2) and head[16:] == (0, 0, 0, 0)
        assert WP.record_plan(EL.EinsumMatmulCircuit(c.k, c.len)).to_bytes() == blob
        assert WP.peek(blob)["n_phases"] == 2 and WP.peek(blob)["n_challenges"] == 2 and WP.peek(blob)["param_hash"] == WP.params_hash(c)
        phases = plan.records[:, 7].tolist()
        assert phases == sorted(phases) and set(phases) == {0, 1}
        kinds = plan.records[:, 0].tolist()
        assert kinds.count(WP.MATMUL) == 1 and kinds.count(WP.INPUT) == 1 and kinds.count(WP.DOT) == 1 and WP.RLC in kinds
        assert all(p == 0 for kd, p in zip(kinds, phases) if kd in (WP.INPUT, WP.MATMUL))
    assert p3.n_records == p17.n_records <= 12
    assert WP.params_hash(c3) != WP.params_hash(c17)
    assert WP.KIND_NAMES[WP.MATMUL] == "matmul" and WP.KIND_NAMES[WP.RLC] == "rlc" and (WP.MATMUL, WP.RLC) == (WP.TBLIDX + 1, WP.TBLIDX + 2)


def test_recorder_still_refuses_what_it_does_not_cover():
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    with pytest.raises(WP.PlanError, match="SumProdCircuit"):
        WP.record_plan(EL.SumProdCircuit(8, 1, 400))
    with pytest.raises(WP.PlanError, match="TransformerSurrogateCircuit"):
        WP.record_plan(EL.TransformerSurrogateCircuit.__new__(EL.TransformerSurrogateCircuit))
    # a value placed in a column of another phase than the one it is available in is refused
    c = EL.EinsumMatmulCircuit(6, 3)
    reg = WP.EinsumRecordingRegion(c)
    cell = reg.put_cell(c.einsums.inputs[0].inner[0][0], 0, WP._Input(0))
    with pytest.raises(WP.PlanError, match="belongs to phase 0"):
        reg.put_cell(c.einsums.inputs[1].inner[0][0], 0, reg.rlc([EL.Val(cell)], 0)[0].v)
    with pytest.raises(WP.PlanError, match="belongs to phase 1"):
        reg.put_cell(c.einsums.inputs[2].inner[0][0], 0, WP._Input(1))


# ---- hand-built plans ---------------------------------------------------------------------------------------------------------------------
def matmul_plan(m, kd, n, k=None, phase=0, n_phases=1, p0=None, p1=None, count=None, n_inputs=None):
    """one MATMUL record: inputs A (m x kd) then B (kd x n) row-major, the product in column 0 from row 0"""
    from ezkl_amd import witness_plan as WP
    if k is None:
        k = max(2, (m * n - 1).bit_length())
    pool = list(range(m * n)) + list(range(m * kd)) + list(range(m * kd, m * kd + kd * n))
    rec = [WP.MATMUL, m * n if count is None else count, kd if p0 is None else p0, n if p1 is None else p1, 0, m * n, m * n + m * kd, phase]
    return WP.WitnessPlan(k, 1, m * kd + kd * n if n_inputs is None else n_inputs, [], [], [rec], [], pool, m * n, 1, b"\0" * 32, n_phases=n_phases)


def matmul_inputs(m, kd, n, seed, extreme=False):
    rng = np.random.default_rng(seed)
    if extreme:                                                    # +-(2^31 - 1) throughout: row 0 of A against column 0 of B is kd * (2^31 - 1)^2
        a = rng.choice([M31, -M31], (m, kd))
        b = rng.choice([M31, -M31], (kd, n))
        a[0, :], b[:, 0] = M31, M31
        if m > 1:
            a[1, :] = -M31
    else:
        a, b = rng.integers(-1000, 1000, (m, kd)), rng.integers(-1000, 1000, (kd, n))
    return a, b, [int(v) for v in a.reshape(-1)] + [int(v) for v in b.reshape(-1)]


def matmul_formula(a, b):
    from ezkl_amd import ezkl_layout as EL
    m, kd, n = a.shape[0], a.shape[1], b.shape[1]
    return [sum(int(a[i, t]) * int(b[t, j]) for t in range(kd)) % EL.R for i in range(m) for j in range(n)]


def rlc_plan(steps, count, k=None, challenge=0, n_challenges=1, input_phase=0, dst_col=1, p1=None):
    """an INPUT record fills column 0 with steps * count values (step-major), an RLC record of phase 1 scans them into column `dst_col`"""
    from ezkl_amd import witness_plan as WP
    m = steps * count
    if k is None:
        k = max(2, (2 * m - 1).bit_length())
    n = 1 << k
    src = list(range(m))
    dst = [dst_col * n + i for i in range(m)] if dst_col else [m + i for i in range(m)]
    pool = src + list(range(m)) + dst
    records = [[WP.INPUT, m, 0, 0, 0, m, 0, input_phase], [WP.RLC, count, challenge, steps if p1 is None else p1, 2 * m, 0, 0, 1]]
    return WP.WitnessPlan(k, 2, m, [], [], records, [], pool, 2 * m, 2, b"\0" * 32, n_challenges=n_challenges, n_phases=2)


def rlc_formula(vals, steps, count, c):
    """out[t] = sum_{u <= t} c^(t - u + 1) * v[u], scan d over vals[t * count + d]"""
    from ezkl_amd import ezkl_layout as EL
    out = [0] * (steps * count)
    for d in range(count):
        for t in range(steps):
            out[t * count + d] = sum(pow(c, t - u + 1, EL.R) * vals[u * count + d] for u in range(t + 1)) % EL.R
    return out


@pytest.mark.parametrize("m,kd,n", [(1, 1, 1), (3, 5, 7)])
def test_hand_built_matmul_plans(m, kd, n):
    from ezkl_amd import witness_plan as WP
    plan = matmul_plan(m, kd, n).validate()
    assert WP.WitnessPlan.from_bytes(plan.to_bytes()) == plan
    for extreme in (False, True):
        a, b, x = matmul_inputs(m, kd, n, 3, extreme)
        cols, _ = WP.run_plan_host(plan, x)
        assert cols[0][:m * n] == matmul_formula(a, b) and not any(cols[0][m * n:])


def test_matmul_operands_at_the_edge_of_the_exact_product_range():
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    m, kd, n = 2, 7, 2
    plan = matmul_plan(m, kd, n)
    a, b, x = matmul_inputs(m, kd, n, 1, extreme=True)
    assert kd * M31 * M31 > 1 << 63, "the sum passes 64 bits"
    cols, _ = WP.run_plan_host(plan, x)
    assert cols[0][:4] == matmul_formula(a, b)
    assert cols[0][0] == kd * M31 * M31 and cols[0][2] == EL.R - kd * M31 * M31
    # an operand equal to 2^31 (either sign, either matrix): reported with record and element, the smallest failing one
    for at, v in ((5, 1 << 31), (m * kd + 3, -(1 << 31)), (0, 1 << 40)):
        bad = list(x)
        bad[at] = v
        bad[m * kd + kd * n - 1] = 1 << 31                         # a later failing operand does not change the report
        with pytest.raises(AssertionError, match=r"einsum operand outside the exact-product range \(matmul record 0, element %d\)" % at):
            WP.run_plan_host(plan, bad)
    ok = list(x)
    ok[5] = -M31
    WP.run_plan_host(plan, ok)


RLC_CHALLENGES = lambda R: [0, 1, R - 1, 0x2b1d3a9f5c7e4d6b8a90123456789abcdef0fedcba9876543210aabbccddeeff % R]


@pytest.mark.parametrize("steps", [1, 15, 16, 17, 33])
def test_hand_built_rlc_plans(steps):
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    R = EL.R
    rng = np.random.default_rng(steps)
    for count in (1, 5):
        plan = rlc_plan(steps, count).validate()
        assert WP.WitnessPlan.from_bytes(plan.to_bytes()) == plan
        x = [int(v) for v in rng.integers(-(1 << 40), 1 << 40, steps * count)]
        for c in RLC_CHALLENGES(R):
            cols, _ = WP.run_plan_host(plan, x, challenges=[c])
            assert cols[0][:steps * count] == [v % R for v in x]
            assert cols[1][:steps * count] == rlc_formula([v % R for v in x], steps, count, c) and not any(cols[1][steps * count:])
        cols, _ = WP.run_plan_host(plan, x, phase=0)
        assert not any(cols[1])


def bad_phase_plans():
    """(what both validators must say, plan)"""
    from ezkl_amd import witness_plan as WP
    _, _, _, _, plan = recorded(6, 3)
    def mutated(edit, **kw):
        q = WP.WitnessPlan.from_bytes(plan.to_bytes())
        q.records = q.records.copy()
        edit(q.records)
        for name, v in kw.items():
            setattr(q, name, v)
        return q
    last = plan.n_records - 1
    def set_phase(ri, ph):
        def edit(r): r[ri, 7] = ph
        return edit
    def set_word(ri, w, v):
        def edit(r): r[ri, w] = v
        return edit
    rlc = plan.records[:, 0].tolist().index(WP.RLC)
    out = [("phases decrease", mutated(set_phase(last, 0))),
           ("phase out of range", mutated(set_phase(last, 2))),
           ("phase out of range", mutated(lambda r: None, n_phases=1)),
           ("challenge index out of range", mutated(set_word(rlc, 2, 2))),
           ("challenge index out of range", mutated(lambda r: None, n_challenges=1)),
           ("bad phase or challenge count", mutated(lambda r: None, n_phases=4)),
           ("a column is written in two phases", rlc_plan(3, 2, dst_col=0)),
           ("challenge index out of range", rlc_plan(3, 2, challenge=1)),
           ("input and matmul records belong to phase 0", rlc_plan(3, 2, input_phase=1)),
           ("input and matmul records belong to phase 0", matmul_plan(2, 2, 2, phase=1, n_phases=2)),
           ("bad matmul shape", matmul_plan(2, 3, 2, p0=0)),
           ("bad matmul shape", matmul_plan(2, 3, 2, p1=0)),
           ("bad matmul shape", matmul_plan(2, 3, 2, p1=3)),                 # count % n != 0
           ("bad matmul shape", matmul_plan(2, 3, 2, p0=4)),                 # a runs past the pool
           ("bad matmul shape", matmul_plan(2, 3, 2, count=8, p1=4)),        # dst + a + b run past the pool
           ("bad rlc shape", rlc_plan(3, 2, p1=0)),
           ("bad rlc shape", rlc_plan(3, 2, p1=1 << 30)),
           ("table index out of range", matmul_plan(2, 3, 2, n_inputs=11))]
    return plan, out


def test_validators_refuse_bad_phases_with_the_same_words():
    import ctypes as C
    from ezkl_amd import native, witness_plan as WP
    L = native.load()
    check = lambda blob: L.ezkl_prover_witness_plan_check(blob, C.c_size_t(len(blob)))
    good, bad = bad_phase_plans()
    for plan in (good, recorded(10, 17)[4], matmul_plan(3, 5, 7), rlc_plan(17, 5)):
        WP.validate(plan)
        assert check(plan.to_bytes()) == 0, L.ezkl_prover_last_error().decode()
    for what, q in bad:
        with pytest.raises(WP.PlanError, match=what) as e:
            WP.validate(q)
        blob = q.to_bytes()
        assert check(blob) == -3, what
        said = L.ezkl_prover_last_error().decode()
        assert str(e.value) == said, (str(e.value), said)
