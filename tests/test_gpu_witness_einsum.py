"""Witness synthesis of the einsum family on the device (csrc/witness.hip: plans with phases, wit_matmul_kernel, wit_rlc_kernel): after the
phase-0 run the first-phase columns are byte-equal to the host layout's, after the phase-1 run -- with the challenges -- the second-phase
columns are, and the first-phase ones are untouched; hand-built matmul and rlc plans agree with the host interpreter at the tile and
chunk edges; an operand outside the exact-product range is reported by name and the process goes on; running the phases out of order
is refused before anything is launched; and create_proof, fed phase by phase from the device, writes the bytes it writes from the host
callback."""
import numpy as np
import pytest

from test_witness_plan_phases_cpu import CHAL, M31, einsum_case, matmul_inputs, matmul_plan, recorded, rlc_plan

pytestmark = pytest.mark.gpu


def _host_columns(c, a, b, chal):
    from ezkl_amd import ezkl_layout as EL
    fn = c.advice_fn(a, b, 6)
    cols = {**fn(0, []), **fn(1, chal)}
    return [EL.ints_to_mont(cols[i]) for i in range(6)]


def _assert_phase(dev, cols, ref, phase, n):
    for i in range(dev.n_advice):
        if dev.column_phase[i] == phase:
            got = cols[i].to_numpy(shape=(n, 4))
            assert got.tobytes() == ref[i].tobytes(), "advice column %d differs on rows %s" % (i, np.nonzero((got != ref[i]).any(1))[0][:8].tolist())


@pytest.mark.parametrize("k,L", [(6, 3), (10, 17), (12, 33)])
def test_device_columns_equal_the_einsum_layout_phase_by_phase(hip, k, L):
    from ezkl_amd import backend as B, ezkl_layout as EL
    R = EL.R
    c, a, b, x, plan = recorded(k, L)
    n = 1 << k
    dev = B.WitnessPlan(plan.to_bytes())
    cols = dev.alloc_columns()
    try:
        assert (dev.n_phases, dev.n_challenges, dev.column_phase) == (2, 2, [0, 0, 1, 1, 0, 1]) and dev.n_records == plan.n_records
        chal = [v % R for v in CHAL]
        ref = _host_columns(c, a, b, chal)
        _, outs = dev.run(x, columns=cols, phase=0)
        assert outs == [] and dev.last["failed"] == 0 and dev.last["device_ms"] > 0
        written = dev.last["cells_written"]
        _assert_phase(dev, cols, ref, 0, n)
        col0 = cols[0].to_numpy(shape=(n, 4)).copy()
        dev.run(None, columns=cols, phase=1, challenges=chal)
        _assert_phase(dev, cols, ref, 1, n)
        assert cols[0].to_numpy(shape=(n, 4)).tobytes() == col0.tobytes() == ref[0].tobytes(), "phase 1 left column 0 alone"
        assert written + dev.last["cells_written"] == plan.n_cells == dev.n_cells and dev.last["failed"] == 0
        assert dev.last["launches"] <= plan.n_records + 4
        # other inputs, other challenges, the same -- now dirty -- columns
        c2, a2, b2, x2 = einsum_case(k, L, seed=5)
        chal2 = [R - 1, 0x0123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef % R]
        ref2 = _host_columns(c, a2, b2, chal2)
        dev.run(x2, columns=cols, phase=0)
        written = dev.last["cells_written"]
        dev.run(None, columns=cols, phase=1, challenges=chal2)
        assert written + dev.last["cells_written"] == plan.n_cells
        for ph in (0, 1):
            _assert_phase(dev, cols, ref2, ph, n)
    finally:
        for col in cols:
            col.free()
        dev.free()


def _device_equals_host(B, plan, x, challenges=None):
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    ref, _ = WP.run_plan_host(plan, x, challenges=challenges)
    dev = B.WitnessPlan(plan.to_bytes())
    cols = dev.alloc_columns()
    try:
        if plan.n_phases == 1:
            dev.run(x, columns=cols)
            written = dev.last["cells_written"]
        else:
            dev.run(x, columns=cols, phase=0)
            written = dev.last["cells_written"]
            dev.run(None, columns=cols, phase=1, challenges=challenges)
            written += dev.last["cells_written"]
        assert written == plan.n_cells
        for d, r in zip(cols, EL.cols_to_mont(ref)):
            got = d.to_numpy(shape=(1 << plan.k, 4))
            assert got.tobytes() == r.tobytes(), "rows %s differ" % np.nonzero((got != r).any(1))[0][:8].tolist()
    finally:
        for col in cols:
            col.free()
        dev.free()


@pytest.mark.parametrize("m,kd,n", [(1, 1, 1), (3, 5, 7), (17, 33, 18), (33, 16, 65)])
def test_hand_built_matmul_plans_on_the_device(hip, m, kd, n):
    from ezkl_amd import backend as B
    plan = matmul_plan(m, kd, n)
    for extreme in (False, True):
        _, _, x = matmul_inputs(m, kd, n, 7, extreme)
        _device_equals_host(B, plan, x)


@pytest.mark.parametrize("count", [1, 5, 67])
def test_hand_built_rlc_plans_on_the_device(hip, count):
    from ezkl_amd import backend as B, ezkl_layout as EL
    R = EL.R
    rng = np.random.default_rng(count)
    for steps in (1, 15, 16, 17, 33, 100):
        plan = rlc_plan(steps, count)
        x = [int(v) for v in rng.integers(-(1 << 40), 1 << 40, steps * count)]
        for c in (0, 1, R - 1):
            _device_equals_host(B, plan, x, [c])


def test_operand_outside_the_exact_product_range_is_reported_and_the_process_goes_on(hip):
    from ezkl_amd import backend as B, ezkl_layout as EL, witness_plan as WP
    c, a, b, x, plan = recorded(10, 17)
    n, L = 1 << 10, 17
    dev = B.WitnessPlan(plan.to_bytes())
    cols = dev.alloc_columns()
    try:
        rec = plan.records[:, 0].tolist().index(WP.MATMUL)
        for at, v in ((L * L + 40, 1 << 31), (5, -(1 << 31))):
            bad = list(x)
            bad[at] = v
            bad[2 * L * L - 1] = 1 << 40                           # a later one does not change the report
            with pytest.raises(B.WitnessError, match=r"einsum operand outside the exact-product range \(matmul record %d, element %d;" % (rec, at)):
                dev.run(bad, columns=cols, phase=0)
            assert dev.last["first"] == (rec, at) and dev.last["failed"] >= 2 and dev.last["cells_written"] < plan.n_cells
            with pytest.raises(AssertionError, match=r"einsum operand outside the exact-product range \(matmul record %d, element %d\)" % (rec, at)):
                WP.run_plan_host(plan, bad, phase=0)
            with pytest.raises(ValueError, match="phase 1 before phase 0"):          # the failed phase 0 does not count
                dev.run(None, columns=cols, phase=1, challenges=CHAL)
        chal = [v % EL.R for v in CHAL]
        ref = _host_columns(c, a, b, chal)
        dev.run(x, columns=cols, phase=0)
        dev.run(None, columns=cols, phase=1, challenges=chal)
        for ph in (0, 1):
            _assert_phase(dev, cols, ref, ph, n)
    finally:
        for col in cols:
            col.free()
        dev.free()


def test_phases_out_of_order_are_refused_before_anything_is_launched(hip):
    from ezkl_amd import backend as B, ezkl_layout as EL
    R = EL.R
    c, a, b, x, plan = recorded(6, 3)
    dev = B.WitnessPlan(plan.to_bytes())
    cols, other = dev.alloc_columns(), dev.alloc_columns()
    try:
        chal = [v % R for v in CHAL]
        with pytest.raises(ValueError, match="phase 1 before phase 0"):
            dev.run(None, columns=cols, phase=1, challenges=chal)
        assert dev.last["launches"] == 0 and dev.last["cells_written"] == 0
        dev.run(x, columns=cols, phase=0)
        with pytest.raises(ValueError, match="phase 1 before phase 0"):              # phase 0 ran on other column pointers
            dev.run(None, columns=other, phase=1, challenges=chal)
        assert dev.last["launches"] == 0
        with pytest.raises(ValueError, match="ezkl_hip_witness_run_phase_dev"):      # the one-call run does not take a plan with phases
            dev.run(x, columns=cols)
        assert dev.last["launches"] == 0
        with pytest.raises(ValueError, match="not a canonical field element"):
            dev.run(None, columns=cols, phase=1, challenges=[chal[0], R])
        assert dev.last["launches"] == 0
        with pytest.raises(ValueError, match="challenge that was not passed"):
            dev.run(None, columns=cols, phase=1, challenges=chal[:1])
        with pytest.raises(ValueError, match="no such phase"):
            dev.run(None, columns=cols, phase=2, challenges=chal)
        dev.run(None, columns=cols, phase=1, challenges=chal)                          # and after all that phase 1 still finds phase 0's cells
        ref = _host_columns(c, a, b, chal)
        for ph in (0, 1):
            _assert_phase(dev, cols, ref, ph, 1 << 6)
    finally:
        for col in cols + other:
            col.free()
        dev.free()


@pytest.mark.parametrize("k,L", [(6, 3), (10, 17)])
def test_create_proof_fed_from_the_device_writes_the_host_callback_bytes(hip, golden_srs, k, L):
    from ezkl_amd import backend as B, ezkl_layout as EL, native as NV, plonk as P
    c, a, b, x, plan = recorded(k, L)
    cs, fixed, copies, rows = c.keygen_inputs(a, b)
    fm = [EL.ints_to_mont(f) for f in fixed]
    if k == 6:
        bg, bgl = B.Bases(golden_srs["g"]), B.Bases(golden_srs["g_lagrange"])
    else:
        bg, bgl = B.gen_srs(k, 0x5eed)
    pk = NV.NativeProvingKey(NV.NativeCircuit(cs), bg, fm, copies)
    fn = c.advice_fn(a, b, cs.n_advice)
    host_fn = lambda phase, chal: {i: EL.ints_to_mont(v) for i, v in fn(phase, chal).items()}
    dev = B.WitnessPlan(plan.to_bytes())
    cols = dev.alloc_columns()
    try:
        ref = NV.create_proof(pk, bg, bgl, host_fn, rng=P.Rng(9))
        got = NV.create_proof(pk, bg, bgl, dev.advice_fn(x, cols), rng=P.Rng(9), device_columns=range(cs.n_advice))
        assert got == ref
        assert sorted(dev.phase_ms) == [0, 1]
        if k == 6:
            from oracle import verifier as V
            from oracle.cpu_backend import OracleBackend
            from test_plonk import setup
            _, vk = P.keygen(cs, OracleBackend(golden_srs["g"], golden_srs["g_lagrange"], 6), fm, copies)
            g1, g2, s_g2 = setup(golden_srs)
            assert V.verify(vk, g1, g2, s_g2, got)
            # the declared and the returned kind must agree: the callback fails, no memory is reinterpreted
            with pytest.raises(RuntimeError):
                NV.create_proof(pk, bg, bgl, host_fn, rng=P.Rng(9), device_columns=[0])
            with pytest.raises(RuntimeError):
                NV.create_proof(pk, bg, bgl, dev.advice_fn(x, cols), rng=P.Rng(9))
            with pytest.raises(ValueError, match="callable"):
                NV.create_proof(pk, bg, bgl, [host_fn(0, [])[0]] * 6, device_columns=[0])
    finally:
        for col in cols:
            col.free()
        dev.free(); bg.free(); bgl.free()
