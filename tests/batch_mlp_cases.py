"""The circuits and inputs of tests/test_batch_mlp_cpu.py, tests/test_gpu_batch_mlp.py and tests/test_gpu_phased_files.py: batched MLPs
(ezkl_layout.BatchMlpCircuit) at the smallest shapes that cross the layout's edges, and the attention head of
tests/test_attention_head_cpu.py.  Decomposition base 128 with two legs: every range-checked value lies in (-16384, 16384)."""
import json

BASE, LEGS = 128, 2
BOUND = BASE ** LEGS
CHAL = [0x1234567890abcdef1234567890abcdef, 0xfedcba0987654321]

TINY = dict(logrows=9, batch=2, weights=[[[1, -2], [0, 1]]], biases=[[1, -1]])
RAGGED = dict(logrows=9, batch=3, weights=[[[1, -2, 3, 0, 1], [0, 1, -1, 2, 0], [0, 1, 1, -3, 2], [1, 2, -1, 0, 1]], [[1, -1, 2, 0], [0, 3, -2, 1]]],
              biases=[[1, -1, 0, 2], [3, -4]], rebase=[4, 1], relu_last=False, relu_first=True)
# 2 x (3 -> 3) at k = 8: the model columns hold 250 rows a block and the layout places more than that, the einsum columns need 27
TWO_BLOCKS = dict(logrows=8, batch=2, weights=[[[1, -1, 0], [0, 1, -1], [-1, 0, 1]]], biases=[[0, -5, 5]])


def batch(spec, num_inner_cols=1):
    from ezkl_amd import ezkl_layout as EL
    spec = dict(spec)
    return EL.BatchMlpCircuit(spec.pop("logrows"), num_inner_cols, spec.pop("batch"), spec.pop("weights"), spec.pop("biases"), BASE, LEGS, **spec)


def attention():
    from ezkl_amd import ezkl_layout as EL
    return EL.AttentionHeadCircuit(10, 4, 4, 2, capacity=6 << 10)


# name -> (the spec, the input matrices the tests run, row-major: the first is the one the GPU file proves; the last holds entries at
# +-(BOUND - 1), the decomposition bound minus one, where the weights and the rebase keep every later value inside the range)
E = BOUND - 1
BATCH_CASES = {
    "tiny": (TINY, [[3, -4, 0, 7], [-100, 50, 25, -25], [E, 8191, -E, -8191]]),
    "ragged": (RAGGED, [[5, -3, 0, 2, 9, -1, -1, 4, 0, 7, 100, -200, 300, 0, -50], list(range(-7, 8)), [E, 0, 0, 0, -E, -E, -E, -E, -E, -E, 0, E, 0, 0, 0]]),
    "two_blocks": (TWO_BLOCKS, [[1, 2, 3, -4, -5, -6], [0] * 6, [E, E, 0, 0, 0, -E]]),
}


def describe_as_mlp(spec, num_inner_cols=1):
    """the batch-1 description of the same network: what the existing "mlp" family reads"""
    j = dict(model="mlp", run_args=dict(logrows=spec["logrows"], num_inner_cols=num_inner_cols, decomp_base=BASE, decomp_legs=LEGS, input_scale=0),
             weights=spec["weights"], biases=spec["biases"], relu_last=spec.get("relu_last", True), relu_first=spec.get("relu_first", False))
    if "rebase" in spec:
        j.update(rebase=spec["rebase"], output_scale=0)
    return j


def write_description(X, circuit, path):
    open(path, "w").write(json.dumps(X.describe(circuit)))
    return str(path)


def data(x):
    return {"input_data": [[float(v) for v in x]]}
