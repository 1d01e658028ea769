"""`ezkl mock` on the GPU (execute.mock -> native.mock -> ezkl_prover_mock -> the check kernels of evalh.hip / vecops.hip), against the
row-by-row big-int MockProver of oracle/mock_prover.py: the same failing gates (gate, row) and lookups (lookup, input, row), the same
totals, and failing copies in the same copy cycles (the GPU compares every cell with its cycle successor, the oracle checks the given
pairs, so their copy records differ but name the same cycles).  Kernel level: the gate check against the sweep (ezkl_hip_eval_h_dev) +
a numpy scan, the lookup miss rows against lookup_multiplicity_batch's `missing`, the copy check against numpy."""
import json
import os
import re
import sys
import time

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tools"))
R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001


@pytest.fixture(scope="module")
def B():
    import ezkl_amd
    from ezkl_amd import backend
    ezkl_amd.init(0)
    return backend


def _mont(cols):
    from ezkl_amd import ezkl_layout as EL
    return EL.cols_to_mont([list(c) for c in cols])


def _cycles(cs, copies):
    """cell (permutation position, row) -> its cycle's label"""
    parent = {}

    def find(x):
        while parent.setdefault(x, x) != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in copies:
        parent[find(tuple(a))] = find(tuple(b))
    return lambda cell: find(tuple(cell))


def _oracle(cs, adv, fixed, inst, copies, chal):
    """oracle failures -> (set of (gate, row)), set of (lookup, input, row), list of copy cells (position, row)"""
    from oracle import mock_prover as MP
    gates, lookups, copy_cells = set(), set(), []
    pos = {kc: i for i, kc in enumerate(cs.perm)}
    for f in MP.check(cs, adv, fixed, inst, copies, chal, max_failures=10**9):
        m = re.match(r"gate (\d+) not satisfied on row (\d+)", f)
        if m:
            gates.add((int(m.group(1)), int(m.group(2))))
            continue
        m = re.match(r"lookup (\d+) input (\d+) row (\d+):", f)
        if m:
            lookups.add((int(m.group(1)), int(m.group(2)), int(m.group(3))))
            continue
        m = re.match(r"copy \((adv|fix|inst)(\d+),(\d+)\) != \((adv|fix|inst)(\d+),(\d+)\)", f)
        assert m, f
        copy_cells.append((pos[(m.group(1), int(m.group(2)))], int(m.group(3))))
    return gates, lookups, copy_cells


def _parity(cs, adv, fixed, inst, copies, chal, records, totals):
    gates, lookups, copy_cells = _oracle(cs, adv, fixed, inst, copies, chal)
    assert sum(totals) <= 10**5                                                  # complete record lists below
    assert {(r[1], r[3]) for r in records if r[0] == 1} == gates and totals[0] == len(gates)
    assert {(r[1], r[2], r[3]) for r in records if r[0] == 2} == lookups and totals[1] == len(lookups)
    cyc = _cycles(cs, copies)
    assert {cyc((r[1], r[3])) for r in records if r[0] == 3} == {cyc(c) for c in copy_cells}
    assert (totals[2] == 0) == (not copy_cells)
    assert totals[2] == sum(r[0] == 3 for r in records)


def _run(cs, adv, fixed, inst, copies, chal=None, cap=10**5):
    """native.mock on int columns; second-phase advice through a callable that records the challenges the GPU drew"""
    from ezkl_amd import native as NV
    seen = {}
    if any(cs.advice_phase):
        def advice(phase, ch):
            seen[phase] = list(ch)
            return {c: m for c, m in zip([i for i in range(cs.n_advice) if cs.advice_phase[i] == phase],
                                         _mont([adv(phase, ch)[i] for i in range(cs.n_advice) if cs.advice_phase[i] == phase]))}
        records, totals = NV.mock(cs, _mont(fixed), copies, advice, instances=inst, seed=3, cap=cap)
        return records, totals, seen.get(1, [])
    records, totals = NV.mock(cs, _mont(fixed), copies, _mont(adv), instances=inst, seed=3, cap=cap)
    return records, totals, []


# ---- 1. the command on the golden k = 6 artefacts ------------------------------------------------------------------------------------
def test_golden_k6_mock_passes_and_a_wrong_output_is_a_copy_into_the_instance_column(B, tmp_path):
    from ezkl_amd import codecs, execute
    wit, model = os.path.join(GOLDEN, "witness_k6.json"), os.path.join(GOLDEN, "model_k6.compiled")
    assert execute.mock(wit, model) == ""
    j = json.load(open(wit))
    j["outputs"][0][0] = codecs.felt_to_hex_le((codecs.felt_from_hex_le(j["outputs"][0][0]) + 1) % R)
    bad = tmp_path / "witness_bad.json"
    bad.write_text(json.dumps(j))
    with pytest.raises(execute.MockError) as e:
        execute.mock(str(bad), model)
    cs = execute._plonk_cs(execute._load_circuit(model)[0])
    inst_pos = [i for i, (kind, c) in enumerate(cs.perm) if kind == "inst"]
    assert e.value.totals[0] == 0 and e.value.totals[1] == 0 and e.value.totals[2] >= 1
    assert any(r[0] == 3 and r[1] in inst_pos for r in e.value.records)
    assert "copy (" in str(e.value) and "instance 0" in str(e.value)


# ---- 2. parity with the oracle's MockProver -------------------------------------------------------------------------------------
def _mlp10():
    from ezkl_amd import ezkl_layout as EL
    rng = np.random.default_rng(5)
    N = 6
    Ws = [rng.integers(-3, 4, (N, N)).tolist() for _ in range(2)]
    bs = [rng.integers(-2, 3, N).tolist() for _ in range(2)]
    c = EL.MlpCircuit(10, 2, Ws, bs, 128, 2)
    x = rng.integers(-3, 4, N).tolist()
    cs, fixed, copies, reg = c.keygen_inputs(x, with_witness=True)
    adv, inst = c.witness_of(reg)
    return cs, [list(map(int, a)) for a in adv], [list(map(int, f)) for f in fixed], inst, copies


def test_mlp_k10_valid_and_20_random_corruptions(B):
    cs, adv, fixed, inst, copies = _mlp10()
    records, totals, _ = _run(cs, adv, fixed, inst, copies)
    assert records == [] and totals == (0, 0, 0)
    rng = np.random.default_rng(11)
    used = [(c, r) for c in range(cs.n_advice) for r in range(cs.usable) if adv[c][r]]
    for t in range(20):
        c, r = used[int(rng.integers(len(used)))]
        bad = [list(a) for a in adv]
        bad[c][r] = (bad[c][r] + int(rng.integers(1, 50))) % R
        records, totals, _ = _run(cs, bad, fixed, inst, copies)
        assert sum(totals) > 0, (c, r)
        _parity(cs, bad, fixed, inst, copies, [], records, totals)


def test_conv_valid_and_a_flipped_cell(B):
    """conv2d_mnist (its 65 537-row table needs k = 17; the oracle is too slow there): a valid witness reports nothing, and every gate record
    of a flipped cell is a gate that really fails on that row (big-int evaluation)"""
    import bench_circuits as BC
    from ezkl_amd import native as NV, plonk as P
    b = BC.build("conv", 17, gpu=B)
    cs, fixed, adv, inst = b["cs"], b["fixed"], b["advice"], b["instances"]
    records, totals = NV.mock(cs, fixed, b["copies"], adv, instances=inst, seed=3)
    assert records == [] and totals == (0, 0, 0)
    col = 0
    row = next(r for r in range(cs.usable) if np.asarray(adv[col][r]).any())
    bad = [np.array(a, copy=True) for a in adv]
    bad[col][row] = P.to_mont((P.from_mont(bad[col][row]) + 1) % R)
    records, totals = NV.mock(cs, fixed, b["copies"], bad, instances=inst, seed=3)
    assert sum(totals) > 0 and any(rec[3] == row for rec in records)
    ip = [list(c) + [0] * cs.n for c in inst]
    for kind, index, sub, r in records:
        if kind == 1:
            q = lambda k_, c_, rot: (P.from_mont(bad[c_][(r + rot) % cs.n]) if k_ == "adv" else P.from_mont(fixed[c_][(r + rot) % cs.n]) if k_ == "fix"
                                     else ip[c_][(r + rot) % cs.n] % R)
            assert P.evaluate(cs.gates[index], q) != 0


def test_einsum_k10_second_phase_parity(B):
    from ezkl_amd import ezkl_layout as EL
    rng = np.random.default_rng(2)
    L = 14
    c = EL.EinsumMatmulCircuit(10, L)
    a, b = rng.integers(-128, 128, (L, L)), rng.integers(-128, 128, (L, L))
    cs, fixed, copies, rows = c.keygen_inputs(a, b)
    fn = c.advice_fn(a, b, cs.n_advice)
    fixed = [list(map(int, f)) for f in fixed]

    def adv(phase, ch):
        d = fn(phase, ch)
        return {i: [int(v) % R for v in d[i]] for i in d}
    records, totals, chal = _run(cs, lambda p, ch: adv(p, ch), fixed, [], copies)
    assert records == [] and totals == (0, 0, 0) and len(chal) == cs.n_challenges
    full = {**adv(0, []), **adv(1, chal)}
    ints = [full[i] for i in range(cs.n_advice)]
    col2 = next(i for i in range(cs.n_advice) if cs.advice_phase[i] == 1 and any(ints[i]))
    row2 = next(r for r in range(cs.usable) if ints[col2][r])

    def tampered(phase, ch):
        d = adv(phase, ch)
        if col2 in d:
            d[col2] = list(d[col2]); d[col2][row2] = (d[col2][row2] + 1) % R
        return d
    records, totals, chal2 = _run(cs, tampered, fixed, [], copies)
    assert chal2 == chal and sum(totals) > 0
    full = {**tampered(0, []), **tampered(1, chal)}
    _parity(cs, [full[i] for i in range(cs.n_advice)], fixed, [], copies, chal, records, totals)


def test_transformer_surrogate_k10_every_tampering(B):
    from ezkl_amd import ezkl_layout as EL
    c = EL.TransformerSurrogateCircuit(10, blocks=2, d=4, einsum_len=3, decomp_base=16, lookup_max=(1 << 10) // 16)
    b = c.build(as_ints=True)
    cs, fixed, copies, inst = b["cs"], [list(f) for f in b["fixed"]], list(b["copies"]), b["instances"]
    U, T = b["info"]["unit_rows"], b["info"]["tiles"]

    def run(edit=None, instances=inst):
        def adv(phase, ch):
            d = {i: list(v) for i, v in b["advice"](phase, ch).items() if cs.advice_phase[i] == phase}
            if edit:
                edit(d)
            return d
        records, totals, chal = _run(cs, adv, fixed, instances, copies)
        full = {**adv(0, []), **adv(1, chal)}
        _parity(cs, [full[i] for i in range(cs.n_advice)], fixed, instances, copies, chal, records, totals)
        return totals
    assert run() == (0, 0, 0)
    probe = {**b["advice"](0, []), **b["advice"](1, [1, 2])}
    col = c.gc.advices[2].inner[1][0].index
    row = next(r for r in range((T - 1) * U, T * U) if probe[col][r])

    def bump(cl, rw):
        def e(d):
            if cl in d:
                d[cl][rw] = (d[cl][rw] + 1) % R
        return e
    assert sum(run(bump(col, row))) > 0                                          # a cell of the last tile of the second block
    col2 = next(i for i in range(cs.n_advice) if cs.advice_phase[i] == 1 and any(probe[i][U:2 * U]))
    row2 = next(r for r in range(U, 2 * U) if probe[col2][r])
    assert sum(run(bump(col2, row2))) > 0                                        # a second-phase cell of a later tile
    tcol = c.gc.advices[5].inner[0][0].index
    trow = next(r for r in range(U) if probe[tcol][r])
    assert run(bump(tcol, trow + U)) == (0, 0, 0)                                # the pick changed in one tile only: nothing to report

    def every_tile(d):
        if tcol in d:
            v = (d[tcol][trow] + 1) % R
            for t in range(T):
                d[tcol][trow + t * U] = v
    assert run(every_tile)[1] > 0                                                # ... in every tile: a lookup failure
    assert run(instances=[[(v + 1) % R for v in inst[0]]])[2] > 0               # wrong public outputs: copies into the instance column


# ---- 3. kernel level ---------------------------------------------------------------------------------------------------------------
def _rand_words(rng, n):
    from ezkl_amd import plonk as P
    return np.stack([P.to_mont(int(v)) for v in rng.integers(0, 5, n)])


def test_check_kernel_matches_the_sweep_per_gate(B):
    import test_mock_cpu as T
    from ezkl_amd import ezkl_layout as EL, plonk as P
    sur = EL.TransformerSurrogateCircuit(10, blocks=2, d=4, einsum_len=3, decomp_base=16, lookup_max=(1 << 10) // 16)
    cs = sur.build(tiles=1)["cs"]
    prog, slots, nc, nch = T.gate_check_program(cs)
    rng = np.random.default_rng(4)
    n = cs.n
    cols = [B.DeviceBuffer.from_numpy(_rand_words(rng, n)) for _ in range(nc)]
    for i in range(nc):                                                          # mostly zero columns: most gates hold, some do not
        if i % 3:
            B.vec_fill(cols[i].ptr, np.zeros(4, np.uint64), n)
    chal = np.stack([P.to_mont(7 + i) for i in range(nch)])
    records, cnt = prog.check_rows([c.ptr for c in cols], chal, slots, 0, n, cap=n * len(slots))
    got = {(r[1], r[3]) for r in records}
    assert len(got) == cnt[0] == len(records)
    want = set()
    for j in slots:                                                              # the sweep of the program ending at slot j, scanned
        sub = B.GraphProgram(cs.k, cs.k)
        sub.constants, sub.rotations, sub.n_intermediates = prog.constants, prog.rotations, prog.n_intermediates
        last = max(i for i, ins in enumerate(prog.code) if ins[1] == j)
        sub.code = prog.code[:last + 1]
        out = B.DeviceBuffer(n * 32)
        sub.evaluate_h([c.ptr for c in cols], chal, out.ptr)
        nz = out.to_numpy(np.uint64, (n, 4)).any(axis=1)
        want |= {(j, r) for r in np.nonzero(nz)[0].tolist()}
    assert got == want and 0 < len(want) < n * len(slots)
    lo, hi = 100, 700                                                            # a row window, and a cap below the count
    records, cnt = prog.check_rows([c.ptr for c in cols], chal, slots, lo, hi, cap=5)
    inside = {x for x in want if lo <= x[1] < hi}
    assert cnt[0] == len(inside) and len(records) == min(5, len(inside)) and {(r[1], r[3]) for r in records} <= inside


def test_lookup_miss_rows_match_the_multiplicity_count(B):
    from ezkl_amd import plonk as P
    rng = np.random.default_rng(6)
    n, u = 1 << 12, (1 << 12) - 6
    tables = [np.stack([P.to_mont(int(v)) for v in rng.integers(0, 300, n)]) for _ in range(3)]
    ins = [[np.stack([P.to_mont(int(v)) for v in rng.integers(0, 400, n)]) for _ in range(q)] for q in (1, 2, 3)]
    dt = [B.DeviceBuffer.from_numpy(t) for t in tables]
    di = [[B.DeviceBuffer.from_numpy(a) for a in l] for l in ins]
    records, cnt = B.lookup_missing_rows([[d.ptr for d in l] for l in di], [d.ptr for d in dt], n, u, cap=3 * 4 * n)
    for l in range(3):
        _, missing = B.lookup_multiplicity_batch([[d.ptr for d in di[l]]], [dt[l].ptr], n, u)
        assert cnt[1 + l] == missing
        tab = {tuple(w) for w in tables[l][:u].tolist()}
        want = {(l, s, r) for s, a in enumerate(ins[l]) for r in range(u) if tuple(a[r].tolist()) not in tab}
        assert {(x[1], x[2], x[3]) for x in records if x[1] == l} == want and len(want) == missing
    assert cnt[0] == sum(cnt[1:]) == len(records)


def test_copy_check_on_random_cycles(B):
    rng = np.random.default_rng(8)
    log_n, m = 10, 5
    n = 1 << log_n
    cells = m * n
    nxt = np.arange(cells, dtype=np.uint32)
    perm = rng.permutation(cells)[:3000]                                         # 300 random cycles of 10 cells
    for cyc in perm.reshape(-1, 10):
        nxt[cyc] = np.roll(cyc, -1)
    vals = rng.integers(0, 1 << 60, (m, n, 4)).astype(np.uint64)
    vals[..., 3] &= np.uint64((1 << 58) - 1)
    for cyc in perm.reshape(-1, 10):                                             # every cycle holds one value ...
        vals[cyc // n, cyc % n] = vals[cyc[0] // n, cyc[0] % n]
    for cyc in perm.reshape(-1, 10)[::7]:                                        # ... except every seventh, broken in one cell
        vals[cyc[3] // n, cyc[3] % n, 0] ^= np.uint64(1)
    dc = [B.DeviceBuffer.from_numpy(vals[c]) for c in range(m)]
    dn = B.DeviceBuffer.from_numpy(nxt)
    records, cnt = B.copy_check([d.ptr for d in dc], dn.ptr, log_n, cap=cells)
    flat = vals.reshape(cells, 4)
    bad = np.nonzero((flat != flat[nxt]).any(axis=1))[0]
    assert {(r[1], r[3]) for r in records} == {(int(t) // n, int(t) % n) for t in bad} and cnt[0] == len(bad) > 0
    records, cnt = B.copy_check([d.ptr for d in dc], dn.ptr, log_n, cap=3)
    assert cnt[0] == len(bad) and len(records) == 3


# ---- 4. cap --------------------------------------------------------------------------------------------------------------------
def test_cap_keeps_exact_totals(B):
    cs, adv, fixed, inst, copies = _mlp10()
    rng = np.random.default_rng(13)
    bad = [list(a) for a in adv]
    used = [(c, r) for c in range(cs.n_advice) for r in range(cs.usable) if adv[c][r]]
    for i in rng.permutation(len(used))[:1000]:
        c, r = used[int(i)]
        bad[c][r] = (bad[c][r] + 1) % R
    records, totals, _ = _run(cs, bad, fixed, inst, copies, cap=16)
    gates, lookups, _ = _oracle(cs, bad, fixed, inst, copies, [])
    assert len(records) == 16 and totals[0] == len(gates) and totals[1] == len(lookups) and sum(totals) > 16
    for rec in records:
        assert (rec[0] == 1 and (rec[1], rec[3]) in gates) or (rec[0] == 2 and (rec[1], rec[2], rec[3]) in lookups) or rec[0] == 3


# ---- 5. scale ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mlp", "einsum"])
def test_k20_mock(B, kind):
    import bench_circuits as BC
    from ezkl_amd import native as NV, plonk as P
    b = BC.build(kind, 20, gpu=B)
    cs = b["cs"]
    live0 = B.pool_stats()["live"]
    t0 = time.perf_counter()
    records, totals = NV.mock(cs, b["fixed"], b["copies"], b["advice"], instances=b["instances"], seed=1)
    print("\n%s k = 20: ezkl_prover_mock %.1f ms" % (kind, 1e3 * (time.perf_counter() - t0)))
    assert records == [] and totals == (0, 0, 0)
    # one flipped cell near the last usable row, in a column whose cell there is constrained
    u = cs.usable
    base = b["advice"]
    cols0 = base(0, []) if callable(base) else {i: a for i, a in enumerate(base)}
    found = None                                                                 # the used cell with the highest row below `usable`
    for c in sorted(cols0):
        nz = np.nonzero(np.asarray(cols0[c]).reshape(-1, 4)[:u].any(axis=1))[0]
        if len(nz) and (found is None or nz[-1] > found[1]):
            found = (c, int(nz[-1]))
    assert found
    c, r = found
    flipped = np.asarray(cols0[c]).reshape(-1, 4).copy()
    flipped[r] = P.to_mont((P.from_mont(flipped[r]) + 1) % R)
    if callable(b["advice"]):
        def advice(phase, ch):
            d = dict(base(phase, ch))
            if c in d:
                d[c] = flipped
            return d
        adv_arg = advice
    else:
        adv_arg = [flipped if i == c else a for i, a in enumerate(b["advice"])]
    records, totals = NV.mock(cs, b["fixed"], b["copies"], adv_arg, instances=b["instances"], seed=1)
    assert sum(totals) > 0 and any(rec[3] == r for rec in records), (found, totals, records[:8])
    assert B.pool_stats()["live"] == live0
