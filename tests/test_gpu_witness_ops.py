"""The kernels of the surrogate's ops (csrc/witness.hip: wit_acc_kernel, the GATHER and CLAMP kinds of wit_elem_kernel, wit_tile_kernel) on
the device: every synthetic plan of tests/witness_synth_ops.py twice into the same columns, the device columns, the status words and the
error text against the closed form; the tile call against np.tile, with what it must leave alone and what it must refuse."""
import re

import numpy as np
import pytest

import witness_synth as S
import witness_synth_ops as O

pytestmark = pytest.mark.gpu
SEEDS = (1, 2)


def _message(plan, refused):
    from ezkl_amd import witness_plan as WP
    ri, el = refused[0]
    assert int(plan.records[ri, 0]) == WP.GATHER
    return re.escape("%s (gather record %d, element %d; %d cells in all)" % (WP.GATHER_ERROR, ri, el, len(refused)))


def _assert_columns(cols, case):
    from ezkl_amd import ezkl_layout as EL
    k = case.plan.k
    got = {}
    for c, want in enumerate(EL.cols_to_mont(case.columns())):
        got[c] = cols[c].to_numpy(shape=(1 << k, 4))
        assert got[c].tobytes() == want.tobytes(), "column %d differs on rows %s" % (c, (got[c] != want).any(1).nonzero()[0][:8].tolist())
    for cell in case.refused_cells:
        assert not got[cell >> k][cell & ((1 << k) - 1)].any(), "a refused lane wrote cell %d" % cell


def _run(B, dev, cols, case):
    plan = case.plan
    if case.refused:
        with pytest.raises(B.WitnessError, match=_message(plan, case.refused)):
            dev.run(case.x, columns=cols)
        assert dev.last["failed"] == len(case.refused) and dev.last["first"] == case.refused[0]
    else:
        _, outs = dev.run(case.x, columns=cols)
        assert outs == case.outputs() and dev.last["failed"] == 0
    assert dev.last["failed"] + dev.last["cells_written"] == plan.n_cells
    _assert_columns(cols, case)


@pytest.mark.parametrize("name", list(O.CASES))
def test_device_columns_equal_the_closed_form(hip, name):
    from ezkl_amd import backend as B
    cols, devs = None, []
    try:
        for seed in SEEDS:                                           # other values into the columns the first run left dirty
            case = O.CASES[name](seed)
            devs.append(B.WitnessPlan(case.plan.to_bytes()))
            cols = cols or devs[-1].alloc_columns()
            _run(B, devs[-1], cols, case)
    finally:
        for c in cols or []:
            c.free()
        for dev in devs:
            dev.free()


def test_gather_failures_are_counted_exactly_and_the_next_run_is_clean(hip):
    from ezkl_amd import backend as B
    bad = O.gather_accounting_case(True, seed=7)
    dev = B.WitnessPlan(bad.plan.to_bytes())
    cols = dev.alloc_columns()
    try:
        _run(B, dev, cols, O.gather_accounting_case(False, seed=6))
        assert bad.refused == [(2, 64), (2, 255), (3, 5), (3, 64), (3, 255), (3, 500)]
        _run(B, dev, cols, bad)
        _run(B, dev, cols, O.gather_accounting_case(False, seed=8))
    finally:
        for c in cols:
            c.free()
        dev.free()


# ---- tiling ---------------------------------------------------------------------------------------------------------------------------------
TILINGS = [(6, 1, 1), (6, 1, 64), (7, 5, 3), (8, 63, 4), (8, 64, 4), (9, 65, 7), (9, 128, 4)]     # the last: U * T = 2^k
N_COLS = 7
PAIRS = [(0, 0), (3, 0), (1, 1), (4, 1), (5, 1)]                   # columns 0 and 1 tiled onto themselves and copied into 3 / 4, 5; 2 and 6 outside


def _random_columns(B, k, seed):
    rng = np.random.default_rng(seed)
    host = [rng.integers(0, 1 << 63, size=(1 << k, 4), dtype=np.uint64) for _ in range(N_COLS)]
    return host, [B.DeviceBuffer.from_numpy(h) for h in host]


@pytest.mark.parametrize("k,U,T", TILINGS)
def test_tiling_equals_np_tile_and_leaves_the_rest_alone(hip, k, U, T):
    from ezkl_amd import backend as B
    host, cols = _random_columns(B, k, 100 * k + U)
    try:
        B.witness_tile(cols, k, U, T, PAIRS)
        want = [h.copy() for h in host]
        for d, s in PAIRS:
            want[d][:U * T] = np.tile(host[s][:U], (T, 1))
        for c in range(N_COLS):
            got = cols[c].to_numpy(shape=(1 << k, 4))
            assert got.tobytes() == want[c].tobytes(), "column %d differs on rows %s" % (c, (got != want[c]).any(1).nonzero()[0][:8].tolist())
        assert (want[2] == host[2]).all() and (want[3][U * T:] == host[3][U * T:]).all()
        assert B.last_kernel_ms("witness_tile") >= 0
    finally:
        for c in cols:
            c.free()


def test_tiling_refusals_launch_nothing(hip):
    import ctypes as C
    from ezkl_amd import backend as B, lib
    k = 7
    host, cols = _random_columns(B, k, 5)
    L = lib.load()
    ptrs = (C.c_void_p * N_COLS)(*[c.ptr for c in cols])

    def call(n_advice, U, T, pairs, columns=ptrs):
        dst, src = ((C.c_uint32 * max(len(pairs), 1))(*[p[i] for p in pairs]) for i in (0, 1))
        return L.ezkl_hip_witness_tile_dev(columns, C.c_uint32(n_advice), C.c_uint32(k), C.c_uint32(U), C.c_uint32(T), dst, src, C.c_uint32(len(pairs)), None)

    try:
        refused = [("U = 0", (N_COLS, 0, 3, PAIRS)), ("T = 0", (N_COLS, 5, 0, PAIRS)), ("U * T > 2^k", (N_COLS, 43, 3, PAIRS)),
                   ("U * T wraps 32 bits", (N_COLS, 1 << 16, 1 << 16, PAIRS)), ("a dst column >= n_advice", (N_COLS, 5, 3, [(N_COLS, 0)])),
                   ("a src column >= n_advice", (3, 5, 3, [(0, 0), (1, 3)])), ("a column twice as dst", (N_COLS, 5, 3, [(3, 0), (3, 1)])),
                   ("a column twice as dst, once onto itself", (N_COLS, 5, 3, [(0, 0), (0, 1)])),
                   ("a src that is another pair's dst", (N_COLS, 5, 3, [(3, 0), (4, 3)])), ("... in the other order", (N_COLS, 5, 3, [(4, 3), (3, 0)])),
                   ("a chain through a self pair's column", (N_COLS, 5, 3, [(1, 0), (2, 1)]))]
        for what, args in refused:
            assert call(*args) == -3, what
            with pytest.raises(ValueError, match="witness_tile"):
                B.witness_tile(cols[:args[0]], k, args[1], args[2], args[3])
        shared = (C.c_void_p * N_COLS)(*[cols[0 if c == 3 else c].ptr for c in range(N_COLS)])
        assert call(N_COLS, 5, 3, [(3, 0)], shared) == -3, "two columns on one buffer"
        for c in range(N_COLS):
            assert cols[c].to_numpy(shape=(1 << k, 4)).tobytes() == host[c].tobytes(), "a refused call wrote column %d" % c
        assert call(N_COLS, 5, 3, []) == 0                           # no pair: nothing to do
        assert call(N_COLS, 5, 3, [(0, 0), (3, 0)]) == 0             # a self pair's column may be copied: its rows [0, U) are only read
        assert (cols[3].to_numpy(shape=(1 << k, 4))[:15] == np.tile(host[0][:5], (3, 1))).all()
    finally:
        for c in cols:
            c.free()


# ---- the surrogate: both phases and the tiling on the device ----------------------------------------------------------------------------------
def _host_and_device(B, k, inputs=None):
    from test_witness_plan_ops_cpu import _surrogate
    host = _surrogate(k).build(gpu=B, inputs=inputs)
    dev = _surrogate(k).build(gpu=B, inputs=inputs, synthesis="device")
    return host, dev


def _assert_device_columns_equal_the_host(host, dev, chal):
    cs = host["cs"]
    want = {**host["advice"](0, []), **host["advice"](1, chal)}
    got = {**dev["advice"](0, []), **dev["advice"](1, chal)}
    assert sorted(got) == sorted(want) == list(range(cs.n_advice)) == dev["device_columns"]
    for i in range(cs.n_advice):
        g = got[i].to_numpy(shape=(cs.n, 4))
        assert g.tobytes() == np.ascontiguousarray(want[i]).tobytes(), "advice column %d differs on rows %s" % (i, (g != want[i]).any(1).nonzero()[0][:8].tolist())
    assert dev["instances"] == host["instances"] and dev["witness"].outputs == host["instances"][0]


@pytest.mark.parametrize("which", ["default", "other"])
def test_surrogate_device_columns_equal_the_host_callable(hip, which):
    from ezkl_amd import backend as B
    from test_witness_plan_ops_cpu import CHAL, _surrogate, other_inputs
    k = 10
    host, dev = _host_and_device(B, k, None if which == "default" else other_inputs(_surrogate(k)))
    try:
        assert dev["info"]["tiles"] >= 3 and dev["info"]["blocks"] == 2
        _assert_device_columns_equal_the_host(host, dev, CHAL)
        _assert_device_columns_equal_the_host(host, dev, [CHAL[1], CHAL[0]])     # other challenges into the same columns
    finally:
        dev["witness"].free()


def test_surrogate_proof_with_the_device_callable_equals_the_host_callable(hip):
    from ezkl_amd import backend as B, ezkl_layout as EL, native as NV, plonk as P
    from oracle import pairing as E, verifier as V
    from oracle.cpu_backend import OracleBackend
    from test_bench_parity import G2
    k = 11
    host, dev = _host_and_device(B, k)
    try:
        cs, copies, fixed = host["cs"], host["copies"], EL.cols_to_mont(host["fixed"], B)
        s = 0x1234567890abcdef1234567890abcdef % P.R
        gb, glb = B.gen_srs(k, s)
        npk = NV.NativeProvingKey(NV.NativeCircuit(cs), gb, fixed, copies)
        by_host = NV.create_proof(npk, gb, glb, host["advice"], rng=P.Rng(5), instances=host["instances"])
        by_device = NV.create_proof(npk, gb, glb, dev["advice"], rng=P.Rng(5), instances=dev["instances"], device_columns=dev["device_columns"])
        assert by_device == by_host
        cpu = OracleBackend(gb.download(), glb.download(), k)
        _, vk = P.keygen(cs, cpu, fixed, copies)
        assert V.verify(vk, (1, 2), G2, E.g2_mul(G2, s), by_device, instances=dev["instances"])
        gb.free(); glb.free()
    finally:
        dev["witness"].free()


def test_a_token_outside_the_table_is_named_and_the_columns_recover(hip):
    from ezkl_amd import backend as B, witness_plan as WP
    from test_witness_plan_ops_cpu import CHAL, _surrogate
    k = 10
    host, dev = _host_and_device(B, k)
    w = dev["witness"]
    try:
        c = _surrogate(k)
        good, bad = c.default_inputs(), c.default_inputs()
        bad[c.d + 3], bad[c.d + 5] = 8, -1
        plan = WP.record_plan(c)
        first = [ri for ri, r in enumerate(plan.records.tolist()) if r[0] == WP.GATHER][0]
        w.set_inputs(bad)
        with pytest.raises(B.WitnessError, match=r"gather index outside the table \(gather record %d, element 3; 4 cells in all\)" % first):
            dev["advice"](0, [])
        assert w.plan.last["failed"] == 4 and w.plan.last["first"] == (first, 3)
        with pytest.raises(ValueError, match="phase 1 before phase 0"):
            dev["advice"](1, CHAL)
        w.set_inputs(good)
        _assert_device_columns_equal_the_host(host, dev, CHAL)
    finally:
        w.free()
