"""The general einsum on the device (csrc/witness.hip wit_dot_wide_kernel, the recorded plans of ezkl_layout.EinsumCircuit and
AttentionHeadCircuit): hand-built DOT records of ONE step agree with the host interpreter cell for cell on both sides of DOT_WIDE_MIN, at
the wave and lane-group edges, on full-range field values, with absent products and absent destinations, and the launch counter tells the
two kernels apart; for every equation of tests/test_einsum_general_cpu.py the device columns equal the host layout phase by phase; and the
attention head's proof made from device synthesis is, at a fixed seed, the proof made from host synthesis byte for byte -- the verifier
accepts it and rejects it with a byte flipped."""
import numpy as np
import pytest

from test_einsum_general_cpu import EQUATIONS, IDS, case, challenges, host_columns

pytestmark = pytest.mark.gpu

K_HAND, N_SRC = 10, 300
COUNTS = [1, 15, 16, 17, 63, 64, 65, 1000]


def _wide_min():
    from ezkl_amd import witness_plan as WP
    return WP.DOT_WIDE_MIN


def dot_plan(p0, count, seed, p1=1, k=K_HAND):
    """N_SRC full-range constants in column 0 (0, 1 and r - 1 among them); one DOT record of `count` dots of p1 steps of p0 products each
    over random cells of them into column 1, with about a tenth of the products and of the destinations absent"""
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    R, NONE = EL.R, WP.NONE
    rng = np.random.default_rng(seed)
    consts = [0, 1, R - 1] + [int.from_bytes(rng.bytes(32), "little") % R for _ in range(N_SRC - 3)]
    src = np.arange(N_SRC, dtype=np.uint32)                                # column 0, rows 0 .. N_SRC - 1
    a = rng.integers(0, N_SRC, (p1 * p0, count)).astype(np.uint32)
    b = rng.integers(0, N_SRC, (p1 * p0, count)).astype(np.uint32)
    gone = rng.random((p1 * p0, count)) < 0.1
    a[gone] = b[gone] = NONE
    dst = ((1 << k) + np.arange(p1 * count, dtype=np.uint32)).reshape(count, p1).T.copy()     # step-major
    no_dst = rng.random((p1, count)) < 0.1
    if count > 1:
        no_dst[:, 0] = False
    else:
        no_dst[:] = False
    dst[no_dst] = NONE
    pool = np.concatenate([src, src, dst.reshape(-1), a.reshape(-1), b.reshape(-1)])
    o = 2 * N_SRC
    records = [[WP.CONST, N_SRC, 0, 0, 0, N_SRC, 0, 0],
               [WP.DOT, count, p0, p1, o, o + p1 * count, o + p1 * count + p1 * p0 * count, 0]]
    n_cells = N_SRC + int((dst != NONE).sum())
    return WP.WitnessPlan(k, 2, 0, [], consts, records, [], pool, n_cells, 2, b"\0" * 32).validate()


def _run_and_compare(B, plan):
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    ref, _ = WP.run_plan_host(plan, [])
    dev = B.WitnessPlan(plan.to_bytes())
    cols = dev.alloc_columns()
    try:
        B.witness_wide_dots(reset=True)
        dev.run([], columns=cols)
        wide = B.witness_wide_dots()
        assert dev.last["cells_written"] == plan.n_cells and dev.last["failed"] == 0
        for i, (d, r) in enumerate(zip(cols, EL.cols_to_mont(ref, B))):
            got = d.to_numpy(shape=(1 << plan.k, 4))
            assert got.tobytes() == r.tobytes(), "column %d: rows %s differ" % (i, np.nonzero((got != r).any(1))[0][:8].tolist())
        return wide
    finally:
        for col in cols:
            col.free()
        dev.free()


@pytest.mark.parametrize("p0", ["1", "min-1", "min", "min+1", "63", "64", "65", "257"])
def test_one_step_dot_records_equal_the_host_interpreter_on_both_kernels(hip, p0):
    from ezkl_amd import backend as B
    m = _wide_min()
    p0 = {"min-1": m - 1, "min": m, "min+1": m + 1}.get(p0) or int(p0)
    for count in COUNTS:
        wide = _run_and_compare(B, dot_plan(p0, count, seed=1000 * p0 + count))
        assert wide == (1 if p0 >= m else 0), "p0 = %d, count = %d ran on the %s kernel" % (p0, count, "wide" if wide else "chunked")


def test_the_counter_and_the_kernel_choice(hip):
    """a record of more than one step keeps the chunked scan whatever its width; the counter accumulates until it is reset"""
    from ezkl_amd import backend as B
    m = _wide_min()
    assert _run_and_compare(B, dot_plan(m + 3, 17, seed=5, p1=2)) == 0
    B.witness_wide_dots(reset=True)
    dev = B.WitnessPlan(dot_plan(m, 5, seed=6).to_bytes())
    cols = dev.alloc_columns()
    try:
        for _ in range(3):
            dev.run([], columns=cols)
        assert B.witness_wide_dots() == 3 and B.witness_wide_dots(reset=True) == 3 and B.witness_wide_dots() == 0
    finally:
        for col in cols:
            col.free()
        dev.free()


@pytest.mark.parametrize("lanes", [1, 2, 4, 8])
def test_many_dots_share_fewer_lanes(hip, lanes):
    """the counts above give every dot 16, 32 or 64 lanes; fewer lanes to a dot -- down to one, a wave of 64 dots -- are chosen only when
    the dots alone fill the device: the smallest such counts, a few dots past a whole wave"""
    from ezkl_amd import backend as B, witness_plan as WP
    p0, count = _wide_min(), WP.DOT_WIDE_FILL // lanes + 3
    assert WP.dot_wide_lanes(count, p0) == lanes and WP.dot_wide_lanes(count // 2, p0) == 2 * lanes
    assert _run_and_compare(B, dot_plan(p0, count, seed=lanes, k=18)) == 1


@pytest.mark.parametrize("eq,dims", EQUATIONS, ids=IDS)
def test_device_columns_equal_the_layout_phase_by_phase(hip, eq, dims):
    from ezkl_amd import backend as B, ezkl_layout as EL, witness_plan as WP
    c, a, b, x = case(eq, dims)
    plan = WP.record_plan(c)
    n, chal = 1 << plan.k, challenges(c)
    dev = B.WitnessPlan(plan.to_bytes())
    cols = dev.alloc_columns()
    try:
        assert (dev.n_phases, dev.n_challenges) == (2, c.analysis.num_output_axes)
        for seed in (1, 5):                                             # then other inputs into the same -- now dirty -- columns
            _, a2, b2, x2 = case(eq, dims, seed)
            first, both = host_columns(c, a2, b2, chal)
            ref = EL.cols_to_mont([both[i] for i in range(6)])
            dev.run(x2, columns=cols, phase=0)
            written = dev.last["cells_written"]
            for i in range(6):
                if dev.column_phase[i] == 0:
                    assert cols[i].to_numpy(shape=(n, 4)).tobytes() == ref[i].tobytes(), "phase 0: advice column %d differs" % i
            dev.run(None, columns=cols, phase=1, challenges=chal)
            assert written + dev.last["cells_written"] == plan.n_cells and dev.last["failed"] == 0
            for i in range(6):
                assert cols[i].to_numpy(shape=(n, 4)).tobytes() == ref[i].tobytes(), "advice column %d differs" % i
    finally:
        for col in cols:
            col.free()
        dev.free()


def test_attention_head_proof_from_device_synthesis_is_the_host_proof(hip):
    from ezkl_amd import backend as B, ezkl_layout as EL, native as NV, plonk as P
    from test_attention_head_cpu import CHAL, K, circuit
    R = EL.R
    host = circuit().build(gpu=B)
    dev = circuit().build(gpu=B, synthesis="device")
    try:
        cs = host["cs"]
        assert dev["instances"] == host["instances"] and dev["device_columns"] == list(range(cs.n_advice))
        chal = [v % R for v in CHAL]
        want = {**host["advice"](0, []), **host["advice"](1, chal)}
        got = {**dev["advice"](0, []), **dev["advice"](1, chal)}
        for i in range(cs.n_advice):
            g = got[i].to_numpy(shape=(cs.n, 4))
            assert g.tobytes() == np.ascontiguousarray(want[i]).tobytes(), "advice column %d differs on rows %s" % (i, (g != want[i]).any(1).nonzero()[0][:8].tolist())
        assert dev["witness"].outputs == host["instances"][0]
        s = 0x1234567890abcdef1234567890abcdef % R
        gb, glb = B.gen_srs(K, s)
        g2, s_g2 = NV.g2_mul_generator(1), NV.g2_mul_generator(s)
        pk = NV.NativeProvingKey(NV.NativeCircuit(cs), gb, EL.cols_to_mont(host["fixed"], B), host["copies"])
        by_host = NV.create_proof(pk, gb, glb, host["advice"], rng=P.Rng(5), instances=host["instances"])
        by_device = NV.create_proof(pk, gb, glb, dev["advice"], rng=P.Rng(5), instances=dev["instances"], device_columns=dev["device_columns"])
        assert by_device == by_host
        assert NV.verify_proof(pk, g2, s_g2, by_device, dev["instances"])
        flipped = bytearray(by_device)
        flipped[len(flipped) // 2] ^= 1
        assert not NV.verify_proof(pk, g2, s_g2, bytes(flipped), dev["instances"])
        gb.free(); glb.free()
    finally:
        dev["witness"].free()
