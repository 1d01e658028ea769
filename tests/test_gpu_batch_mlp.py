"""The two-phase plans of the batched MLPs and the attention head on the device (tests/batch_mlp_cases.py): both phases replayed at
fixed challenges equal the host layout word for word, and the plan's outputs gathered after phase 0 (ezkl_hip_witness_outputs_dev,
backend.WitnessPlan.outputs) are the outputs its last phase gathers and the cells themselves -- refused, with nothing launched, before
phase 0 has run and on other columns than it ran on."""
import numpy as np
import pytest

import batch_mlp_cases as F
from test_batch_mlp_cpu import NAMES, _columns, built

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", NAMES + ["attention"])
def test_both_phases_equal_the_host_layout_and_the_outputs_come_after_phase_0(hip, name):
    from ezkl_amd import backend as B, ezkl_layout as EL
    R = EL.R
    c, b, plan, x = built(name)
    n, chal = 1 << plan.k, [v % R for v in F.CHAL]
    ref = EL.cols_to_mont(_columns(b, chal))
    dev = B.WitnessPlan(plan.to_bytes())
    cols, other = dev.alloc_columns(), dev.alloc_columns()
    try:
        assert (dev.n_phases, dev.n_challenges, dev.n_outputs) == (2, 2, len(c.outputs)) and dev.lookup_phases in ([], [0])
        B.kernel_ms_stats("witness_outputs", reset=True)
        with pytest.raises(ValueError, match="before phase 0 has run"):
            dev.outputs(cols)
        dev.run(x, columns=cols, phase=0)
        written = dev.last["cells_written"]
        for i in range(dev.n_advice):
            if dev.column_phase[i] == 0:
                assert cols[i].to_numpy(shape=(n, 4)).tobytes() == ref[i].tobytes(), "phase 0: advice column %d differs" % i
        with pytest.raises(ValueError, match="other columns than the ones phase 0 ran on"):
            dev.outputs(other)
        with pytest.raises(ValueError, match="other columns"):
            dev.outputs(cols[1:] + cols[:1])
        assert B.kernel_ms_stats("witness_outputs")[1] == 0, "a refused call launches nothing"
        after_first = dev.outputs(cols)
        assert B.kernel_ms_stats("witness_outputs")[1] == 1 and dev.last_outputs_ms >= 0
        M_inv = pow(1 << 256, -1, R)
        by_cell = [int.from_bytes(cols[cell >> plan.k].words(cell & (n - 1)).tobytes(), "little") * M_inv % R for cell in plan.outputs.tolist()]
        _, with_last = dev.run(None, columns=cols, phase=1, challenges=chal)
        assert written + dev.last["cells_written"] == plan.n_cells and dev.last["failed"] == 0
        assert after_first == with_last == by_cell == c.outputs == b["instances"][0]
        assert dev.outputs(cols) == after_first                             # and after the last phase as well
        for i in range(dev.n_advice):
            got = cols[i].to_numpy(shape=(n, 4))
            assert got.tobytes() == ref[i].tobytes(), "advice column %d differs on rows %s" % (i, (got != ref[i]).any(1).nonzero()[0][:8].tolist())
        # a refused phase 0 takes the outputs away again: the cells are not a witness
        if name != "attention":
            past = list(x)
            past[0] = F.BOUND
            with pytest.raises(B.WitnessError):
                dev.run(past, columns=cols, phase=0)
            with pytest.raises(ValueError, match="before phase 0 has run"):
                dev.outputs(cols)
    finally:
        for col in cols + other:
            col.free()
        dev.free()


def test_the_device_witness_classes_read_their_outputs_in_one_gather(hip):
    from ezkl_amd import backend as B
    c, b, plan, x = built("ragged")
    made = F.batch(F.BATCH_CASES["ragged"][0]).build(gpu=B, synthesis="device", inputs=x)
    try:
        B.kernel_ms_stats("witness_outputs", reset=True)
        assert made["instances"] == b["instances"] == [made["witness"].read_outputs()]
        assert B.kernel_ms_stats("witness_outputs")[1] == 1
        assert isinstance(np.asarray(made["instances"][0], dtype=object)[0], int)
    finally:
        made["witness"].free()
