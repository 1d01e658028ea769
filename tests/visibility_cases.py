"""What tests/test_visibility_cpu.py and tests/test_gpu_visibility.py share: the 18 visibility triples of the MLP family, the base case
(the k = 6 fixture shape: Gemm 3 -> 4 + ReLU, 16 parameters), the smallest circuit whose committed parameters span two columns, and the
two file forms of a circuit -- this package's JSON description and a `model.compiled`-shaped node graph as codecs.read_compiled_circuit
returns one."""
import itertools

INPUT, PARAMS, OUTPUT = ("Private", "Public", "KZGCommit"), ("Private", "Fixed", "KZGCommit"), ("Public", "KZGCommit")
TRIPLES = list(itertools.product(INPUT, PARAMS, OUTPUT))
DEFAULT = ("Private", "Private", "Public")
assert len(TRIPLES) == 18 and DEFAULT in TRIPLES

K, WIDTH, BASE, LEGS = 6, 2, 128, 2
BOUND = BASE ** LEGS                                            # |value| < BOUND wherever the layout decomposes it
WEIGHTS, BIASES = [[1, -2, 3], [0, 5, -1], [2, 2, 2], [-3, 1, 4]], [1, -40, 3, 0]
X = [3, -2, 7]
# signed permutation rows, no bias: every value of the circuit is an input or its negation, so the inputs may sit at the bound
UNIT_WEIGHTS, UNIT_BIASES = [[1, 0, 0], [0, 1, 0], [0, 0, -1], [-1, 0, 0]], [0, 0, 0, 0]
EDGE_INPUTS = [[0, 0, 0], [BOUND - 1, -(BOUND - 1), 1], [-1, -BOUND + 1, BOUND - 1], [-5, 0, -7]]
OVER_INPUTS = [[BOUND, 0, 0], [0, -BOUND, 0], [0, 0, BOUND + 1]]


def ids(tri):
    return "-".join(tri)


def mlp(tri, weights=WEIGHTS, biases=BIASES, k=K, w=WIDTH):
    from ezkl_amd import ezkl_layout as EL
    return EL.MlpCircuit(k, w, [weights], [biases], BASE, LEGS, visibility=tri)


def run_args(tri, k=K, w=WIDTH):
    return dict(logrows=k, num_inner_cols=w, decomp_base=BASE, decomp_legs=LEGS, input_visibility=tri[0], param_visibility=tri[1], output_visibility=tri[2])


def description(tri, weights=WEIGHTS, biases=BIASES, k=K, w=WIDTH):
    return {"model": "mlp", "run_args": run_args(tri, k, w), "weights": [weights], "biases": [biases]}


def two_column():
    """the smallest square layer whose flattened parameters exceed one column at the smallest k it fits in: k = 7 has 2^7 - 6 = 122 rows
    a column, 11 x 11 + 11 = 132 parameters.  Small weights of both signs; -> (weights, biases, x, k, num_inner_cols)"""
    m = 11
    weights = [[((3 * r + 5 * c) % 7) - 3 for c in range(m)] for r in range(m)]
    biases = [(r % 5) - 2 for r in range(m)]
    return weights, biases, [(i % 9) - 4 for i in range(m)], 7, 2


def compiled(tri, total_const_size, total_assignments, weights=WEIGHTS, biases=BIASES, k=K, w=WIDTH):
    """a parsed `model.compiled` of the same circuit: Input -> Einsum "mk,nk->mn" with a constant [n, k] -> Add of a constant [1, n] ->
    LeakyReLU slope 0, every scale 0, and the GraphSettings fields execute reads"""
    from ezkl_amd import ezkl_layout as EL
    n_out, n_in = len(weights), len(weights[0])
    felt = lambda v: v % EL.R
    const = lambda vals, dims: dict(kind="Constant", quantized_values=dict(inner=[felt(v) for v in vals], dims=dims))
    nodes = {0: dict(opkind=dict(kind="Input", datum_type="F32", decomp=True), out_scale=0, inputs=[], out_dims=[1, n_in], idx=0),
             1: dict(opkind=const([v for row in weights for v in row], [n_out, n_in]), out_scale=0, inputs=[], out_dims=[n_out, n_in], idx=1),
             2: dict(opkind=const(biases, [1, n_out]), out_scale=0, inputs=[], out_dims=[1, n_out], idx=2),
             3: dict(opkind=dict(kind="Linear", op="Einsum", equation="mk,nk->mn"), out_scale=0, inputs=[(0, 0), (1, 0)], out_dims=[1, n_out], idx=3),
             4: dict(opkind=dict(kind="Linear", op="Add"), out_scale=0, inputs=[(3, 0), (2, 0)], out_dims=[1, n_out], idx=4),
             5: dict(opkind=dict(kind="Linear", op="LeakyReLU", slope=0.0), out_scale=0, inputs=[(4, 0)], out_dims=[1, n_out], idx=5)}
    model = dict(nodes=nodes, inputs=[0], outputs=[(5, 0)], visibility=dict(input=tri[0], params=tri[1], output=tri[2]))
    sizes = [n for v, n in zip(tri, (n_in, n_out * n_in + n_out, n_out)) if v == "KZGCommit"]
    settings = dict(run_args=run_args(tri, k, w), total_assignments=total_assignments, total_const_size=total_const_size,
                    required_range_checks=[(-1, 1), (0, BASE - 1)], required_lookups=[], num_dynamic_lookups=0, num_shuffles=0,
                    einsum_params=dict(equations=[], total_einsum_col_size=0), model_input_scales=[0], model_output_scales=[0],
                    module_sizes=dict(polycommit=sizes, poseidon=[0, [0]]))
    return dict(model=model, settings=settings)
