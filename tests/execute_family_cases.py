"""The circuits and inputs of tests/test_execute_families_cpu.py and tests/test_gpu_execute_families.py: one conv, norm and pooled-classifier
description per shape, each with explicit parameters (not the seeded ones), the inputs the tests run, and what a test needs to compute
the lookup statistics on its own."""
import json

import numpy as np


def conv_k6():
    """the k = 6 circuit of tests/test_witness_plan_lookup_cpu.py `_case_b`: every kernel entry 3, an image of four constant 3 x 3 quadrants --
    the lookup inputs are 27 * level over a Div{4} table of +-100"""
    from ezkl_amd import ezkl_layout as EL
    rng = np.random.default_rng(2)
    fc_w, fc_b = rng.integers(-5, 6, (2, 4)), rng.integers(-9, 10, 2)
    return EL.ConvMnistCircuit(logrows=6, image=6, kernel=3, out_channels=1, stride=3, classes=2, lookup_range=(-100, 100), denom=4, decomp_base=16,
                               decomp_legs=2, capacity=220, kernels=np.full((1, 3, 3), 3), conv_bias=[0], fc_w=fc_w, fc_b=fc_b)


def quadrants(levels):
    return np.kron(np.array(levels).reshape(2, 2), np.ones((3, 3), np.int64)).reshape(-1).tolist()


def conv_k10():
    """tests/test_witness_plan_lookup_cpu.py `_case_a`: kernels in [-3, 3], a Div{4} table of +-700, with a conv bias of its own"""
    from ezkl_amd import ezkl_layout as EL
    rng = np.random.default_rng(1)
    return EL.ConvMnistCircuit(logrows=10, image=8, kernel=3, out_channels=2, stride=2, classes=3, lookup_range=(-700, 700), denom=4, decomp_base=32,
                               decomp_legs=2, kernels=rng.integers(-3, 4, (2, 3, 3)), conv_bias=[5, -7], fc_w=rng.integers(-12, 13, (3, 18)),
                               fc_b=rng.integers(-40, 41, 3))


def norm(layer_norm):
    from ezkl_amd import ezkl_layout as EL
    return EL.NormCircuit(9, 2, 3000, 2, 4, layer_norm=layer_norm)


def pool(kind):
    from ezkl_amd import ezkl_layout as EL
    rng = np.random.default_rng(5)
    return EL.PoolClassifierCircuit(10, 2, 12000, pool=kind, kernels=rng.integers(-4, 5, (2, 3, 3)), conv_bias=rng.integers(-8, 9, 2),
                                    fc_w=rng.integers(-4, 5, (4, 18)), fc_b=rng.integers(-16, 17, 4))


def flat_image_past_the_table(circuit):
    """a constant image whose greatest relu output lies past the circuit's lookup table and inside its decomposition range"""
    sums = np.asarray(circuit.kernels).reshape(circuit.oc, -1).sum(axis=1)
    for v in range(1, 4096):
        conv = [int(s) * v + int(b) for s, b in zip(sums, circuit.conv_bias)]
        if max(conv) > circuit.lookup_range[1] and all(abs(c) < circuit.base ** circuit.legs for c in conv):
            return [v] * circuit.n_inputs
    raise AssertionError("no such image")


_IMG8 = lambda seed, hi: np.random.default_rng(seed).integers(0, hi, 64).tolist()
# name -> (make the circuit, the inputs the tests run: the first is the one the GPU file proves, an input the circuit must refuse)
CASES = {
    "conv_k6": (conv_k6, [quadrants((0, 1, 2, 3)), quadrants((3, 3, 1, 2)), [0] * 36], quadrants((0, 1, 2, 4))),        # 27 * 4 = 108 > 100
    "conv_k10": (conv_k10, [_IMG8(1, 4), _IMG8(2, 4), [0] * 64], flat_image_past_the_table(conv_k10())),
    "norm_softmax": (lambda: norm(False), [[1, 5, -3, 7, 0, 0, 2, 9], [-20, -30, -25, -21, 4, 3, 2, 1], [0] * 8], [0, 300, 0, 0, 0, 0, 0, 0]),      # 0 - 300 < -255
    "norm_layer_norm": (lambda: norm(True), [[1, 5, -3, 7, 0, 0, 2, 9], [-20, -30, -25, -21, 4, 3, 2, 1], [0] * 8], None),
    "pool_max": (lambda: pool("max"), [_IMG8(11, 16), _IMG8(12, 16), [0] * 64], None),
    "pool_sum": (lambda: pool("sum"), [_IMG8(11, 16), _IMG8(12, 16), [0] * 64], None),
}


def expected_stats(name, circuit, x):
    """(min_lookup_inputs, max_lookup_inputs) worked out without the layout engine: the relu outputs of the convolution (the Div table's
    inputs) from numpy, x - max(row) for the softmax (the exp table's inputs), nothing for the circuits without a static lookup"""
    if name.startswith("conv"):
        img = np.asarray(x, np.int64).reshape(circuit.image, circuit.image)
        s, K, st = circuit.slides, circuit.kernel, circuit.stride
        conv = [int((img[i * st:i * st + K, j * st:j * st + K] * np.asarray(circuit.kernels[o])).sum()) + int(circuit.conv_bias[o])
                for o in range(circuit.oc) for i in range(s) for j in range(s)]
        act = [max(v, 0) for v in conv]
        return min(0, *act), max(0, *act)
    if name == "norm_softmax":
        rows = np.asarray(x, np.int64).reshape(circuit.rows, circuit.length)
        sub = (rows - rows.max(axis=1, keepdims=True)).reshape(-1).tolist()
        return min(0, *sub), max(0, *sub)
    return 0, 0


def write_description(X, circuit, path, **scales):
    open(path, "w").write(json.dumps(X.describe(circuit, **scales)))
    return str(path)


def data(x):
    return {"input_data": [[float(v) for v in x]]}
