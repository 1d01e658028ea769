"""The command bodies around the prove hot path, with the reference's names and argument meaning
(/root/reference/src/execute.rs): artefact FILES in, artefact files out, everything O(n) on the GPU through libezkl_prover.so.

    gen_srs(srs_path, logrows)                                                  execute.rs gen_srs -> pfsys::srs::gen_srs (srs.rs:13-16)
    setup(compiled_circuit, srs_path, vk_path, pk_path)                         execute.rs:1543-1572 -> pfsys::create_keys (mod.rs:376-400)
    gen_witness(compiled_circuit, data, output, vk_path, srs_path)               execute.rs:577-660 -> GraphCircuit::forward (graph/mod.rs:1734-1849)
    prove(witness, compiled_circuit, pk_path, proof_path, srs_path, check_mode)  execute.rs:1575-1627 -> create_proof_circuit (mod.rs:404-489)
    mock(witness, compiled_circuit)                                              execute.rs:1280-1305 -> MockProver::run(..).verify()
    verify(proof_path, compiled_circuit, pk_path, srs_path)                      execute.rs:1651-1722 -> verify_proof_circuit (mod.rs:557-590)
    swap_proof_commitments(proof_path, witness_path)                             execute.rs:1629-1650 -> pfsys::swap_proof_commitments (mod.rs:492-554)

File formats are the reference's: kzg*.srs / pk.key / vk.key in halo2 raw bytes, witness.json (GraphWitness), proof.json (Snark) and
`model.compiled` -- the bincode of ezkl's GraphCircuit (node graph + GraphSettings), read by codecs.read_compiled_circuit: on the
reference's fixture `prove` runs from the reference's artefact files alone (tests/test_execute.py).  What a compiled circuit may
CONTAIN here is the op family ezkl_layout.MlpCircuit lays out (Input -> Gemm as Einsum "mk,nk->mn" + bias + LeakyReLU slope 0): ezkl's
general layout lives in 6.8k lines of Rust (out of scope) and any other graph is refused by name.
VISIBILITY, the MLP family in both its forms (run_args.input_visibility / param_visibility / output_visibility of a description, the
model's own of a model.compiled): the input Private, Public or KZGCommit; the parameters Private, Fixed or KZGCommit; the output Public or
KZGCommit -- 18 triples, Private / Private / Public being the default and what it always was, byte for byte.  A Public input shares the
instance column with the output (input first); Fixed parameters are constants of the key; a KZGCommit tensor is laid into unblinded advice
columns that come first in the system, so its commitment -- which gen_witness writes into witness.json as processed_*.polycommit -- is
one of the first points of every proof (swap_proof_commitments; ezkl_layout.MlpCircuit has the layout).  Anything Hashed, a Fixed input or
output and a Private output are refused by name by every entry point.  A description that asked for another triple used to be laid out
with the default one, silently; it now gets the circuit it asks for.  On the fixture model that layout reproduces the reference's pk.key bit for bit (tests/test_ezkl_circuit.py).  A JSON
description of the same family ({"model": "mlp", "run_args": {...}, "weights": [...], "biases": [...]}) is accepted as well; with
"rebase": [d per layer] every Gemm is wrapped in the RebaseScale division ezkl puts around it at non-zero scales (layouts.rs:219-267 `div`):
the input is then quantized at run_args.input_scale and the outputs are reported at input_scale + sum(param_scale - log2 d), or at
"output_scale" where a divisor is no power of two.
Three more families are read as JSON descriptions, chosen by "model" through the table FAMILIES (`describe` writes one from a circuit):
    {"model": "conv", "run_args": {...}, "image", "kernel", "out_channels", "stride", "classes", "lookup_range": [lo, hi], "denom", ["capacity"],
     "kernels": [oc][K][K], "conv_bias": [oc], "fc_w": [classes][oc * slides^2], "fc_b": [classes]}                  -> ezkl_layout.ConvMnistCircuit
    {"model": "pool_classifier", "run_args": {...}, "image", "kernel", "out_channels", "stride", "pool_size", "pool_stride", "classes",
     "pool": "max" | "sum", "capacity", and the same four arrays}                                                     -> PoolClassifierCircuit
    {"model": "norm", "run_args": {...}, "rows", "length", "input_scale", "output_scale", "eps", "layer_norm", "lookup_range", "capacity"}   -> NormCircuit
with run_args = logrows, num_inner_cols, decomp_base, decomp_legs and optionally input_scale / output_scale (the witness file's scales,
default 0); private input, private parameters and public output only in THESE families -- any other visibility is refused by name, a
malformed field by a ValueError that names it.  setup, gen_witness, mock, prove, verify and Prover treat them as they treat the MLP.
Two families have SECOND-PHASE advice -- their matmuls are Freivalds einsums over the circuit's own configuration, two challenges -- and
live in the table PHASED_FAMILIES:
    {"model": "mlp_batch", "run_args": {logrows, num_inner_cols, decomp_base, decomp_legs[, input_scale, param_scale]}, "batch": m, "weights", "biases",
     ["rebase", "output_scale", "relu_last", "relu_first", "capacity"]}      -> ezkl_layout.BatchMlpCircuit: the MLP description on m >= 2 input rows (ezkl's batch_size;
                                                                                the scales and the rebase divisors follow the MLP description's rules)
    {"model": "attention", "run_args": {...}, "n", "e", "d", "capacity", "input_scale", "output_scale", "eps", "score_div", "lookup_range", "Wq", "Wk", "Wv"}
                                                                             -> AttentionHeadCircuit
A circuit is phased when its constraint system has advice beyond phase 0 (_phased), and every entry point then takes one path for
both: setup writes a two-phase witness plan next to the key; gen_witness runs the layout's first phase, or replays phase 0 of the plan
and gathers the outputs (ezkl_hip_witness_outputs_dev) -- the outputs and every static lookup live in phase 0; mock, prove and Prover
hand native.mock / native.create_proof a callable advice(phase, challenges), which on the device keeps the phase-0 columns as they
are and replays phase p > 0 with the prover's challenges into the session's one resident column set; verify is host only, as ever.
Both take num_inner_cols = 1: the einsum layout places one entry a row.
The standalone einsum and the transformer surrogate, the SortTopk / SumProd / ScatterGather circuits and sharded / group proving have
no description: "unsupported compiled circuit".
Errors surface as exceptions with the reference's wording where it has one."""
import collections
import json
import os

import numpy as np

from . import backend as B
from . import codecs, ezkl_layout as EL, native as NV
from . import witness_plan as WP


class CheckMode:
    SAFE, UNSAFE = "SAFE", "UNSAFE"


POLYCOMMIT_BLINDING = 5                  # vk.cs().blinding_factors() of this gate family: no advice column is queried at more than 3 rotations


def _read_compiled(path, any_visibility=False):
    """the reference's own `model.compiled` (bincode of GraphCircuit, codecs.read_compiled_circuit) or this package's JSON description
    -> (what it says of the op family, as plain data; the parsed file).  settings: the file's GraphSettings (the JSON description has
    none); any_visibility: see _mlp_of_graph."""
    raw = open(path, "rb").read()
    if raw[:1] == b"{":
        j = json.loads(raw)
        family = _family(j.get("model"))
        if family is None:                                                           # (the standalone einsum and the surrogate among them)
            raise ValueError("unsupported compiled circuit: %r" % j.get("model"))
        return dict(family.describe(j), family=j["model"]), j
    c = codecs.read_compiled_circuit(raw)
    return _describe_compiled(c, any_visibility), c


def _describe_compiled(c, any_visibility=False):
    """a parsed `model.compiled` (codecs.read_compiled_circuit: "model", the node graph with its visibilities, and "settings") as the
    plain data of the MLP family"""
    weights, biases, relu_last, relu_first, n_inputs = _mlp_of_graph(c["model"], any_visibility)
    st, in_op = c["settings"], c["model"]["nodes"][c["model"]["inputs"][0]]["opkind"]
    return dict(weights=weights, biases=biases, relu_last=relu_last, relu_first=relu_first, rebase=None, n_inputs=n_inputs, run_args=st["run_args"], settings=st,
                total_assignments=st["total_assignments"], in_scale=st["model_input_scales"][0], out_scale=st["model_output_scales"][0],
                datum_type=in_op.get("datum_type", "F32"), input_decomp=in_op.get("decomp", True), visibility=c["model"]["visibility"], family="mlp")


def _describe_mlp(j):
    """{"model": "mlp", ...} as plain data (the module's text has the fields)"""
    ra, weights = j["run_args"], j["weights"]
    scale = ra.get("input_scale", 0) if not weights else 0                      # a Gemm-free graph keeps its input scale (ezkl's default: 7)
    in_scale = out_scale = scale
    rebase = j.get("rebase")
    if rebase is not None:                                                       # every Gemm wrapped in a RebaseScale: the scales are the run args'
        rebase = [int(d) for d in rebase]
        if len(rebase) != len(weights) or any(not 1 <= d < 1 << 32 for d in rebase):
            raise ValueError("compiled circuit: \"rebase\" takes one divisor in [1, 2^32) per layer")
        in_scale = ra.get("input_scale", 0)
        if "output_scale" in j:
            out_scale = int(j["output_scale"])
        elif all(d & (d - 1) == 0 for d in rebase) and "param_scale" in ra:       # a layer adds the parameter scale, its rebase takes log2 d off
            out_scale = in_scale + sum(ra["param_scale"] - (d.bit_length() - 1) for d in rebase)
        else:
            raise ValueError("compiled circuit: \"output_scale\" is required where a rebase divisor is not a power of two (or run_args has no param_scale)")
    return dict(weights=weights, biases=j["biases"], relu_last=j.get("relu_last", True), relu_first=j.get("relu_first", False), rebase=rebase,
                n_inputs=j.get("n_inputs", len(weights[0][0]) if weights else None), run_args=ra, settings=None,
                total_assignments=j.get("total_assignments"), in_scale=in_scale, out_scale=out_scale, datum_type="F32", input_decomp=True,
                visibility=dict(input=ra.get("input_visibility", "Private"), params=ra.get("param_visibility", "Private"),
                                output=ra.get("output_visibility", "Public")))


def _build_mlp(d):
    st, ra = d["settings"], d["run_args"]
    if st is not None:
        want = [(-1, 1), (0, ra["decomp_base"] - 1)]
        if [tuple(x) for x in st["required_range_checks"]] != want or st["required_lookups"] or st["num_dynamic_lookups"] or st["num_shuffles"] \
                or st["einsum_params"]["equations"]:
            raise ValueError("unsupported compiled circuit: its settings ask for arguments outside the MLP family")
    vis = EL.visibility_triple(d["visibility"])                                  # (anything outside the family's triples: refused by name)
    # the constant cells of a compiled file with Fixed parameters are the file's count; a description's are counted by a dummy pass
    consts = st["total_const_size"] if st is not None and vis[1] == "Fixed" else None
    circuit = EL.MlpCircuit(ra["logrows"], ra["num_inner_cols"], d["weights"], d["biases"], ra["decomp_base"], ra["decomp_legs"],
                            total_assignments=d["total_assignments"], relu_last=d["relu_last"], n_inputs=d["n_inputs"], relu_first=d["relu_first"],
                            rebase=d["rebase"], visibility=vis, total_const_size=consts)
    if st is not None and [int(v) for v in st["module_sizes"]["polycommit"]] != circuit.settings.polycommit_sizes:
        raise ValueError("unsupported compiled circuit: its module sizes %s are not those of its visibilities %s"
                         % (list(st["module_sizes"]["polycommit"]), circuit.settings.polycommit_sizes))
    # a module column holds 2^k - 6 values because the system had 5 blinding factors when it was configured; gen_witness commits at that
    # split too.  A finished system with another count would put the unusable rows elsewhere: refused, never committed at the wrong split
    if circuit.gc.polycommit and circuit.gc.cs.blinding_factors() != POLYCOMMIT_BLINDING:
        raise ValueError("unsupported compiled circuit: %d blinding factors where the KZG-committed columns were sized for %d"
                         % (circuit.gc.cs.blinding_factors(), POLYCOMMIT_BLINDING))
    return circuit


_REQUIRED = object()
_PARAMETER_ARRAYS = ("kernels", "conv_bias", "fc_w", "fc_b")
_CIRCUIT_RUN_ARGS = ("logrows", "num_inner_cols", "decomp_base", "decomp_legs")      # the run_args that are constructor arguments of a circuit


def _int_field(j, name, least=None, default=_REQUIRED, prefix=""):
    """the integer field `name` of a JSON description, at least `least`; a missing, non-integer or smaller one is a ValueError naming it"""
    v = j.get(name, default)
    if v is _REQUIRED:
        raise ValueError("compiled circuit: \"%s%s\" is missing" % (prefix, name))
    if isinstance(v, bool) or not isinstance(v, int) or (least is not None and v < least):
        raise ValueError("compiled circuit: \"%s%s\" must be an integer%s" % (prefix, name, "" if least is None else " >= %d" % least))
    return v


def _range_field(j, name):
    v = j.get(name)
    if not isinstance(v, (list, tuple)) or len(v) != 2 or any(isinstance(x, bool) or not isinstance(x, int) for x in v) or v[0] > v[1]:
        raise ValueError("compiled circuit: \"%s\" must be [lo, hi], two integers with lo <= hi" % name)
    return (v[0], v[1])


def _run_args(j):
    """the run_args of a JSON description that states its layout: logrows, num_inner_cols, decomp_base and decomp_legs as checked
    integers over the object as it stands; private input, private parameters and a public output -- any other visibility is refused by
    name"""
    ra = j.get("run_args")
    if not isinstance(ra, dict):
        raise ValueError("compiled circuit: \"run_args\" must be an object")
    for what, key, want in (("input", "input_visibility", "Private"), ("params", "param_visibility", "Private"), ("output", "output_visibility", "Public")):
        v = ra.get(key, want)
        if v != want:
            named = v if isinstance(v, str) else next(iter(v), "?") if isinstance(v, dict) else repr(v)
            raise ValueError("unsupported visibility: %s is %s (the %s family takes a private input, private parameters and a public output)"
                             % (what, named, j["model"]))
    run = {name: _int_field(ra, name, least, prefix="run_args.") for name, least in (("logrows", 1), ("num_inner_cols", 1), ("decomp_base", 2), ("decomp_legs", 1))}
    return dict(ra, **run)


def _describe_layout(j, fields, n_inputs):
    """what the conv, pool_classifier and norm descriptions share: run_args (logrows, num_inner_cols, decomp_base, decomp_legs; input_scale
    and output_scale are the witness file's scales, default 0), private input, private parameters and a public output -- any other
    visibility is refused by name --, and the family's own fields, each read by its reader; n_inputs(fields): the length of the input vector.
    -> plain data; "fields": the circuit's arguments"""
    ra = _run_args(j)
    in_scale, out_scale = (_int_field(ra, name, default=0, prefix="run_args.") for name in ("input_scale", "output_scale"))
    f = {name: read(j, name) for name, read in fields}
    return dict(run_args=ra, settings=None, in_scale=in_scale, out_scale=out_scale, datum_type="F32", n_inputs=n_inputs(f),
                visibility=dict(input="Private", params="Private", output="Public"), fields=f)


def _parameter_field(j, name):
    if name not in j:
        raise ValueError("compiled circuit: \"%s\" is missing" % name)
    return j[name]                                                               # its shape and entries: the circuit's constructor (ValueError naming the array)


def _optional(read):
    return lambda j, name: read(j, name) if j.get(name) is not None else None


def _choice_field(*choices):
    def read(j, name):
        if j.get(name) not in choices:
            raise ValueError("compiled circuit: \"%s\" must be one of %s" % (name, ", ".join("\"%s\"" % c for c in choices)))
        return j[name]
    return read


def _eps_field(j, name):
    v = j.get(name)
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not v > 0:
        raise ValueError("compiled circuit: \"%s\" must be a positive number" % name)
    return float(v)


def _bool_field(j, name):
    if not isinstance(j.get(name), bool):
        raise ValueError("compiled circuit: \"%s\" must be true or false" % name)
    return j[name]


_positive = lambda j, name: _int_field(j, name, 1)
_PARAMETERS = [(name, _parameter_field) for name in _PARAMETER_ARRAYS]
_CONV_FIELDS = [(name, _positive) for name in ("image", "kernel", "out_channels", "stride", "classes", "denom")] + \
               [("lookup_range", _range_field), ("capacity", _optional(_positive))] + _PARAMETERS
_POOL_FIELDS = [(name, _positive) for name in ("image", "kernel", "out_channels", "stride", "pool_size", "pool_stride", "classes", "capacity")] + \
               [("pool", _choice_field("max", "sum"))] + _PARAMETERS
_NORM_FIELDS = [(name, _positive) for name in ("rows", "length", "input_scale", "output_scale", "capacity")] + \
               [("eps", _eps_field), ("layer_norm", _bool_field), ("lookup_range", _range_field)]


def _configured(model, make):
    """the circuit, or a ValueError: what the configuration itself refuses (a geometry that does not fit, a kernel larger than its image)
    is refused as a field is"""
    try:
        return make()
    except (AssertionError, ZeroDivisionError, IndexError) as e:
        raise ValueError("compiled circuit: the \"%s\" description cannot be configured: %s" % (model, e or type(e).__name__)) from None


def _build_layout(d):
    """the circuit of a description that states its layout: the family's cross-field checks, then its class over the validated fields --
    the family's own ("fields") and the four of run_args that configure a circuit, by the constructor's parameter names"""
    family = _family(d["family"])
    family.check(d)
    args = dict(d["fields"], **{name: d["run_args"][name] for name in _CIRCUIT_RUN_ARGS})
    return _configured(d["family"], lambda: family.circuit(**args))


def _conv_fits(d):
    f = d["fields"]
    if f["kernel"] > f["image"]:
        raise ValueError("compiled circuit: \"kernel\" is larger than \"image\"")


def _pool_fits(d):
    f = d["fields"]
    _conv_fits(d)
    if f["pool_size"] > (f["image"] - f["kernel"]) // f["stride"] + 1:
        raise ValueError("compiled circuit: \"pool_size\" is larger than the convolution's output")


_ATTENTION_WEIGHTS = ("Wq", "Wk", "Wv")
_ATTENTION_FIELDS = [(name, _positive) for name in ("n", "e", "d", "capacity", "input_scale", "output_scale", "score_div")] + \
                    [("eps", _eps_field), ("lookup_range", _range_field)] + [(name, _parameter_field) for name in _ATTENTION_WEIGHTS]


def _one_inner_column(d):
    """the einsum layout's own rule, named as a field: a wider block folds num_inner_cols entries a row in its RLC gate, which neither
    ezkl_layout.EinsumCircuit lays out nor a witness plan's RLC record states"""
    if d["run_args"]["num_inner_cols"] != 1:
        raise ValueError("compiled circuit: \"run_args.num_inner_cols\" must be 1 in the \"%s\" family: %s" % (d["family"], EL.EINSUM_WIDTH_ERROR))


def _integer_rows(j, name, depth):
    """the field `name`: a non-empty list, nested `depth` deep, of int64 integers (rows of one level may differ in length: the circuit's
    constructor holds the shapes together); anything else is a ValueError naming the field"""
    def ok(v, depth):
        if depth == 0:
            return not isinstance(v, bool) and isinstance(v, int) and -(1 << 63) <= v < 1 << 63
        return isinstance(v, list) and len(v) > 0 and all(ok(x, depth - 1) for x in v)
    if name not in j:
        raise ValueError("compiled circuit: \"%s\" is missing" % name)
    if not ok(j[name], depth):
        raise ValueError("compiled circuit: \"%s\" must be a non-empty list, nested %d deep, of integers that fit int64" % (name, depth))
    return j[name]


def _describe_mlp_batch(j):
    """{"model": "mlp_batch", ...} as plain data: the MLP description's fields, read by _describe_mlp -- its rules for the scales and
    the rebase divisors hold --, on a batch of "batch" input rows"""
    ra = _run_args(j)
    m = _int_field(j, "batch", 1)
    weights, biases = _integer_rows(j, "weights", 3), _integer_rows(j, "biases", 2)
    if len(biases) != len(weights):
        raise ValueError("compiled circuit: \"biases\" takes one vector per matrix of \"weights\"")
    for name in ("relu_last", "relu_first"):
        if name in j:
            _bool_field(j, name)
    for name in ("input_scale", "param_scale"):
        if name in ra:
            _int_field(ra, name, prefix="run_args.")
    if "rebase" in j and j["rebase"] is not None and (not isinstance(j["rebase"], list) or any(isinstance(v, bool) or not isinstance(v, int) for v in j["rebase"])):
        raise ValueError("compiled circuit: \"rebase\" takes one divisor in [1, 2^32) per layer")
    if "output_scale" in j:
        _int_field(j, "output_scale")
    d = _describe_mlp(dict(j, run_args=ra))
    fields = dict({name: d[name] for name in ("weights", "biases", "relu_last", "relu_first", "rebase")}, batch=m, capacity=_optional(_positive)(j, "capacity"))
    return dict(d, n_inputs=m * len(weights[0][0]), fields=fields)


def _mlp_batch_scales(run_args, fields, output_scale):
    """what a written "mlp_batch" description says of its scales, by _describe_mlp's rules: they go with the rebase divisors -- a circuit
    that rescales nothing states neither divisors nor an output scale --, and run_args has no output_scale"""
    del run_args["output_scale"]
    rebase = fields.pop("rebase")
    if any(d != 1 for d in rebase):
        fields.update(rebase=list(rebase), output_scale=output_scale)


def _forward_layout(d, x):
    """gen_witness on the host for a circuit that states its `layout`: its own synthesis, the outputs it ties to the instance column and
    the statistics the layout kept.  What the layout asserts of a witness (a lookup input outside its table, a value beyond the
    decomposition range) is a ValueError with the layout's words."""
    circuit = _family(d["family"]).build(d)
    try:
        reg = circuit.synthesize(x, witness=True)
    except AssertionError as e:
        raise ValueError(str(e) or "the layout refused the input") from None
    return [EL.signed(v) for v in circuit.outputs], (reg.min_lookup_inputs, reg.max_lookup_inputs), _max_range_size(circuit)


def _max_range_size(circuit):
    """the largest hi - lo of the circuit's range checks (GraphWitness max_range_size)"""
    return max((hi - lo for lo, hi in circuit.gc.settings.required_range_checks), default=0)


def _forward_mlp(d, x):
    """gen_witness on the host for the MLP family: the integer arithmetic of its ops in Python lists, with the range checks the layout
    would make.  -> (outputs, (0, 0): no lookups, max_range_size)"""
    weights, biases, relu_last, relu_first = d["weights"], d["biases"], d["relu_last"], d["relu_first"]
    base, legs = d["run_args"]["decomp_base"], d["run_args"]["decomp_legs"]
    limit = base ** legs
    ranged = False
    def decomposed(vals, where):
        nonlocal ranged
        ranged = True
        for v in vals:
            if abs(v) >= limit:
                raise ValueError("%s: %d exceeds the decomposition range (-%d^%d, %d^%d)" % (where, v, base, legs, base, legs))
    if d["input_decomp"]:
        decomposed(x, "input")
    if relu_first:
        decomposed(x, "LeakyReLU input")
        x = [v if v > 0 else 0 for v in x]
    rebase = d["rebase"] or [1] * len(weights)
    for li, (W, bvec) in enumerate(zip(weights, biases)):
        x = [sum(a * w for a, w in zip(x, row)) for row in W]
        if rebase[li] != 1:                              # RebaseScale around the Gemm: `div` claims the rounded quotient and decomposes it
            if any(abs(v) >= 1 << 52 for v in x):
                raise ValueError("layer %d: %s" % (li, EL.DIV_ERROR))
            x = [EL.round_div(v, rebase[li]) for v in x]
            decomposed(x + [rebase[li]], "rebase quotient of layer %d" % li)        # (the divisor: d - |remainder| is decomposed too)
        x = [v + bvec[o] for o, v in enumerate(x)]
        if li + 1 < len(weights) or relu_last:
            decomposed(x, "LeakyReLU input of layer %d" % li)
            x = [v if v > 0 else 0 for v in x]
    decomposed(x, "output")                              # `output` range-checks the outputs and the instance cells (layouts.rs:6740-6779)
    return x, (0, 0), (base - 1) if ranged else 0


# THE families a JSON description may name: how its fields are read, how the circuit is built from them, and gen_witness's forward pass on
# the host.  (The reference's own model.compiled is the MLP family's.)  The standalone einsum, the transformer surrogate and the SortTopk,
# SumProd and ScatterGather circuits are in neither table: naming one is "unsupported compiled circuit".
# A family that states its layout also names its circuit class -- built from the validated fields by the constructor's parameter names
# (_build_layout, after the family's cross-field `check`) and written back from the class's `config()` (describe; `scales` adjusts what
# is written of the scales) --; the MLP family reads the reference's files too and has a builder and no writer of its own.
Family = collections.namedtuple("Family", "describe build forward circuit check scales", defaults=(None,) + (lambda *args: None,) * 2)
FAMILIES = {
    "mlp": Family(_describe_mlp, _build_mlp, _forward_mlp),
    "conv": Family(lambda j: _describe_layout(j, _CONV_FIELDS, lambda f: f["image"] ** 2), _build_layout, _forward_layout, EL.ConvMnistCircuit, _conv_fits),
    "pool_classifier": Family(lambda j: _describe_layout(j, _POOL_FIELDS, lambda f: f["image"] ** 2), _build_layout, _forward_layout,
                              EL.PoolClassifierCircuit, _pool_fits),
    "norm": Family(lambda j: _describe_layout(j, _NORM_FIELDS, lambda f: f["rows"] * f["length"]), _build_layout, _forward_layout, EL.NormCircuit),
}
# the families whose circuits lay Freivalds einsums over their own configuration -- second-phase advice, two-phase plans (_phased) --,
# read, built and run as the ones above are (`_family` looks a name up in both tables); the host forward pass is the layout's first phase
PHASED_FAMILIES = {
    "mlp_batch": Family(_describe_mlp_batch, _build_layout, _forward_layout, EL.BatchMlpCircuit, _one_inner_column, _mlp_batch_scales),
    "attention": Family(lambda j: _describe_layout(j, _ATTENTION_FIELDS, lambda f: f["n"] * f["e"]), _build_layout, _forward_layout,
                        EL.AttentionHeadCircuit, _one_inner_column),
}
_DESCRIBED = {family.circuit: name for name, family in {**FAMILIES, **PHASED_FAMILIES}.items() if family.circuit is not None}


def _family(name):
    """the Family a description's "model" names, or None"""
    return (FAMILIES.get(name) or PHASED_FAMILIES.get(name)) if isinstance(name, str) else None


def describe(circuit, input_scale=0, output_scale=0):
    """the JSON description (a dict) of a ConvMnistCircuit, a PoolClassifierCircuit, a NormCircuit, an AttentionHeadCircuit or a
    BatchMlpCircuit: what `_load_circuit` builds the same circuit from -- same plan_identity, same settings.  It is the circuit's
    `config()`: run_args holds the fields of _CIRCUIT_RUN_ARGS and the two scales, every other field stands under its own name, arrays as
    lists; the seed is left out, the parameter arrays it seeded are all there.  (A BatchMlpCircuit that rescales nothing is at scale 0,
    as the MLP description is: input_scale and output_scale go with its rebase divisors.)"""
    name = _DESCRIBED.get(type(circuit))
    if name is None:
        raise ValueError("no JSON description for a %s" % type(circuit).__name__)
    fields = {key: np.asarray(v).tolist() if isinstance(v, (np.ndarray, tuple)) else v for key, v in circuit.config().items() if key != "seed"}
    run_args = dict({key: fields.pop(key) for key in _CIRCUIT_RUN_ARGS}, input_scale=input_scale, output_scale=output_scale)
    _family(name).scales(run_args, fields, output_scale)
    return dict(model=name, run_args=run_args, **fields)


def _load_circuit(path):
    """the compiled circuit (_read_compiled) as the circuit of its family (FAMILIES) -> (circuit, the parsed file)"""
    d, parsed = _read_compiled(path)
    return _family(d["family"]).build(d), parsed


def _mlp_of_graph(model, any_visibility=False):
    """the op family ezkl_layout.MlpCircuit lays out, read off ezkl's node graph: Input -> (Einsum "mk,nk->mn" with a constant [n, k]
    -> Add of a constant [1, n] -> LeakyReLU slope 0)*, at scale 0, with one of the family's visibility triples (ezkl_layout.VISIBILITIES).  A LeakyReLU slope 0 may
    sit straight on the input, and the layer list may be EMPTY: Input -> LeakyReLU -> output is examples/onnx/1l_relu (BASELINE
    configs[0]; with no Gemm nothing is rescaled, so that graph may carry any ONE scale -- ezkl's default input scale is 7).
    any_visibility (gen_witness, which names a refused visibility itself): the visibilities are the caller's business.
    -> (weights, biases, relu_last, relu_first, n_inputs)"""
    nodes, vis = model["nodes"], model["visibility"]
    if len(model["inputs"]) != 1 or len(model["outputs"]) != 1:
        raise ValueError("unsupported compiled circuit: visibility / arity")
    if not any_visibility:
        EL.visibility_triple(vis)                                                   # a triple outside the family's is refused by name
    def const(idx, dims_ok):
        op = nodes[idx]["opkind"]
        if op["kind"] != "Constant" or not dims_ok(op["quantized_values"]["dims"]):
            raise ValueError("unsupported compiled circuit: node %d is not the expected constant" % idx)
        q = op["quantized_values"]
        return [EL.signed(v) for v in q["inner"]], q["dims"]
    cur = model["inputs"][0]
    order = sorted(k for k in nodes if nodes[k]["opkind"]["kind"] == "Linear")
    gemm_free = all(nodes[k]["opkind"]["op"] == "LeakyReLU" for k in order)
    scales = {n["out_scale"] for n in nodes.values()}
    if nodes[cur]["opkind"]["kind"] != "Input" or (scales != {0} and not (gemm_free and len(scales) == 1)):
        raise ValueError("unsupported compiled circuit: input node / non-zero scales")
    n_inputs = 1
    for d in nodes[cur]["out_dims"]:
        n_inputs *= d
    weights, biases, relu_last, relu_first, i = [], [], False, False, 0
    if order and nodes[order[0]]["opkind"]["op"] == "LeakyReLU":
        n = nodes[order[0]]
        if n["opkind"]["slope"] != 0.0 or n["inputs"] != [(cur, 0)]:
            raise ValueError("unsupported compiled circuit: LeakyReLU with a slope")
        cur, i, relu_first = order[0], 1, True
    while i < len(order):
        n = nodes[order[i]]
        if n["opkind"]["op"] != "Einsum" or n["opkind"]["equation"] != "mk,nk->mn" or n["inputs"][0] != (cur, 0):
            raise ValueError("unsupported compiled circuit: node %d" % order[i])
        w, dims = const(n["inputs"][1][0], lambda d: len(d) == 2)
        weights.append([w[r * dims[1]:(r + 1) * dims[1]] for r in range(dims[0])])
        cur, i = order[i], i + 1
        n = nodes[order[i]] if i < len(order) else None
        if n is None or n["opkind"]["op"] != "Add" or n["inputs"][0] != (cur, 0):
            raise ValueError("unsupported compiled circuit: a Gemm without its bias")
        biases.append(const(n["inputs"][1][0], lambda d: d[-1] == dims[0])[0])
        cur, i = order[i], i + 1
        relu_last = False
        if i < len(order) and nodes[order[i]]["opkind"]["op"] == "LeakyReLU":
            n = nodes[order[i]]
            if n["opkind"]["slope"] != 0.0 or n["inputs"] != [(cur, 0)]:
                raise ValueError("unsupported compiled circuit: LeakyReLU with a slope")
            cur, i, relu_last = order[i], i + 1, True
    if model["outputs"][0] != (cur, 0) or not (weights or relu_first):
        raise ValueError("unsupported compiled circuit: output node")
    return weights, biases, relu_last, relu_first, n_inputs


G2_GENERATOR = ((0x1800deef121f1e76426a00665e5c4479674322d4f75edadd46debd5cd992f6ed, 0x198e9393920d483a7260bfb731fb5d25f1aa493335a9e71297e485b7aef312c2),
                (0x12c85ea5db8c6deb4aab71808dcb408fe3d1e7690c43d37b4ce6cc0166fa7daa, 0x090689d0585ff075ec9e99ad690c3395bc4b313370b38ef355acdadcd122975b))


def gen_srs(srs_path, logrows, secret=None):
    """`ezkl gen-srs` (/root/reference/src/execute.rs gen_srs -> pfsys::srs::gen_srs, src/pfsys/srs.rs:13-16 -> ParamsKZG::setup): an INSECURE
    test SRS from a secret s -- g[i] = s^i G, g_lagrange[i] = L_i(s) G and s_g2 = [s] g2, all on the device (the G1 sets by
    backend.gen_srs, the G2 point by ezkl_hip_msm_g2) -- written in halo2's raw-bytes layout.  secret=None draws s from OS entropy."""
    R_ = EL.R
    if secret is None:
        secret = int.from_bytes(os.urandom(40), "little")
    secret %= R_
    mont_q = lambda v: np.frombuffer((v * (1 << 256) % B._Q).to_bytes(32, "little"), np.uint64)
    mont_r = lambda v: np.frombuffer((v * (1 << 256) % R_).to_bytes(32, "little"), np.uint64)
    g2 = np.concatenate([mont_q(c) for c in (G2_GENERATOR[0][0], G2_GENERATOR[0][1], G2_GENERATOR[1][0], G2_GENERATOR[1][1])])
    g, gl = B.gen_srs(logrows, secret)                       # first: it refuses a secret inside the domain (ValueError) before any device work
    try:
        s_g2 = B.msm_g2(g2[None], mont_r(secret)[None])
        data = codecs.write_srs(dict(k=logrows, g=g.download(), g_lagrange=gl.download(), g2=g2.tobytes(), s_g2=s_g2.tobytes()))
    finally:
        g.free(); gl.free()
    open(srs_path, "wb").write(data)
    return len(data)


class SrsError(ValueError):
    """an SRS file that must not be used: .report is what backend.check_srs (or the loaders' point check, in the same shape) found"""

    def __init__(self, msg, report):
        super().__init__(msg)
        self.report = report


SRS_CHECK_POLICIES = ("points", "full", "off")


def _srs_policy():
    """EZKL_SRS_CHECK: what the loaders check before a point set of an SRS file is used.  "points" (the default): every point that will be
    used is a point of G1 (Bases.check); "full": also the structure of the whole file (backend.check_srs); "off": nothing."""
    policy = os.environ.get("EZKL_SRS_CHECK", "points")
    if policy not in SRS_CHECK_POLICIES:
        raise ValueError("EZKL_SRS_CHECK must be one of points, full, off; got %r" % policy)
    return policy


def check_srs(srs_path, structure=True, seed=None):
    """The whole SRS file, whatever circuit it will later serve: every point of both sets on the device, and with structure=True that g is
    a sequence of powers of the secret s_g2 carries (a random combination and one pairing), that g_lagrange is the Lagrange basis of g
    and that neither set holds an identity (backend.check_srs).  Returns the report; a file that fails raises SrsError, which carries
    it, with a message such as "g_lagrange[513]: point not on the curve"."""
    report = B.check_srs(codecs.read_srs(open(srs_path, "rb").read()), seed=seed, structure=structure)
    if not report["ok"]:
        raise SrsError(report["reason"], report)
    return report


def _read_srs(srs_path, logrows):
    """the SRS file, parsed; one smaller than the circuit is refused.  Under EZKL_SRS_CHECK=full the whole file is held to
    backend.check_srs here, before any of it is used."""
    policy = _srs_policy()
    srs = codecs.read_srs(open(srs_path, "rb").read())
    if srs["k"] < logrows:
        raise ValueError("SRS too small: k=%d < logrows=%d" % (srs["k"], logrows))
    if policy == "full":
        report = B.check_srs(srs)
        if not report["ok"]:
            raise SrsError(report["reason"], report)
    return srs


def _srs_bases(points, name):
    """THE way a point set of an SRS file becomes a resident base set in this module: uploaded, and unless EZKL_SRS_CHECK=off every point
    of it -- exactly the points that will be used -- checked on the device before anything else touches the handle.  A bad point raises
    SrsError naming the set, the index and the reason; nothing stays resident then."""
    policy = _srs_policy()
    b = B.Bases(np.ascontiguousarray(points))
    if policy == "off":
        return b
    try:
        found = b.check()
    except BaseException:
        b.free()
        raise
    if found["bad"]:
        b.free()
        why = "%s[%d]: %s" % (name, found["first_bad"], B.POINT_REASONS[found["reason"]])
        raise SrsError(why, dict(k=None, key=None, points={name: found}, powers=None, lagrange=None, g2=None, ok=False, reason=why))
    return b


def _update_secret(secret):
    """the t of update_srs: None draws 64 bytes of OS entropy, reduced mod r and redrawn if 0; an explicit one must be an integer in [1, r)"""
    if secret is None:
        while True:
            t = int.from_bytes(os.urandom(64), "little") % EL.R
            if t:
                return t
    if isinstance(secret, bool) or not isinstance(secret, (int, np.integer)):
        raise ValueError("update_srs: the secret must be an integer in [1, r), got %s" % type(secret).__name__)
    if not 1 <= int(secret) < EL.R:
        raise ValueError("update_srs: the secret must be an integer in [1, r)")
    return int(secret)


def update_srs(srs_in, srs_out, secret=None):
    """One step of an updatable SRS: multiply a fresh secret t into the file srs_in -- g'[i] = t^i g[i], g_lagrange' rebuilt from g',
    s_g2' = [t] s_g2, all on the device (backend.update_srs) -- and write the result to srs_out in the same layout.  Whoever made srs_in
    knows its secret s; the new file's secret is s t, which nobody knows once one updater has discarded their t.  secret=None draws t
    from OS entropy; an explicit one must be an integer in [1, r) and is refused (ValueError) before any device work otherwise.  The
    input is read as every loader reads an SRS file: EZKL_SRS_CHECK applies to it.  -> dict(k, t_g2: [t] g2 as hex, what
    verify_srs_update needs next to the two files, sha256_in, sha256_out).  t itself is not returned and not written anywhere."""
    import hashlib
    t = _update_secret(secret)
    srs = _read_srs(srs_in, 0)
    g = _srs_bases(srs["g"], "g")                             # the points the update multiplies, held to the loaders' policy
    try:
        new, proof = B.update_srs(srs, t, g=g)
    finally:
        g.free()
    data = codecs.write_srs(new)
    open(srs_out, "wb").write(data)
    return dict(k=new["k"], t_g2=proof["t_g2"].hex(), sha256_in=hashlib.sha256(open(srs_in, "rb").read()).hexdigest(),
                sha256_out=hashlib.sha256(data).hexdigest())


def verify_srs_update(old_path, new_path, t_g2):
    """Is the file new_path the file old_path updated by the secret behind t_g2 (the hex string, or the 128 bytes, update_srs returned)?
    Both files whole: same k and g2, both pass the structural check of check_srs, t_g2 is a point of G2, and e(g[1], t_g2) ==
    e(g'[1], g2) (backend.verify_srs_update).  Returns the report; a failure raises SrsError, which carries it, with a message that
    begins with the step that failed.  It does not prove that the updater knew or discarded their secret."""
    if isinstance(t_g2, str):
        t_g2 = bytes.fromhex(t_g2)
    old, new = (codecs.read_srs(open(p, "rb").read()) for p in (old_path, new_path))
    report = B.verify_srs_update(old, new, dict(t_g2=t_g2))
    if not report["ok"]:
        raise SrsError(report["reason"], report)
    return report


def _downsized(srs, logrows):
    """`params.downsize(logrows)` of an SRS larger than the circuit -> the two resident base sets (g, g_lagrange): the coefficient basis
    is truncated, the Lagrange basis of the smaller domain is rebuilt on the device by an inverse NTT over G1 (ezkl_hip_bases_downsize =
    halo2's g_to_lagrange)"""
    big = _srs_bases(srs["g"][:1 << logrows], "g")
    try:
        return big.downsize(logrows)
    finally:
        big.free()


def load_params_prover(srs_path, logrows):
    """execute.rs:1739-1750: read the SRS and, if the file is larger than the circuit (the normal case with a shared kzg22.srs),
    downsize it (_downsized); -> host arrays"""
    srs = _read_srs(srs_path, logrows)
    if srs["k"] > logrows:
        g, gl = _downsized(srs, logrows)
        try:
            srs = dict(k=logrows, g=g.download(), g_lagrange=gl.download(), g2=srs["g2"], s_g2=srs["s_g2"])
        finally:
            g.free(); gl.free()
    return srs


def setup(compiled_circuit, srs_path, vk_path, pk_path, sample_input=None):
    """keygen_vk + keygen_pk on the GPU, keys written in halo2's raw-bytes layout"""
    circuit, j = _load_circuit(compiled_circuit)
    srs = load_params_prover(srs_path, circuit.k)
    x = sample_input if sample_input is not None else [0] * circuit.n_inputs
    cs, fixed, copies, reg = circuit.keygen_inputs(x)          # synthesis without witness values: selectors + copy constraints
    bg = _srs_bases(srs["g"], "g")
    try:
        pk = NV.NativeProvingKey(NV.NativeCircuit(cs), bg, EL.cols_to_mont(fixed, B), copies)
        pk.set_selectors(reg.selector_rows())
        data = pk.to_bytes()
    finally:
        bg.free()
    open(pk_path, "wb").write(data)
    vk_len = 7 + 64 * (cs.n_fixed + len(cs.perm)) + cs.n_selectors * ((cs.n + 7) // 8)
    open(vk_path, "wb").write(data[:vk_len])                   # vk.key is the prefix of pk.key
    # the witness plan `prove` replays on the device: an OPTIONAL artefact, written after the keys.  A circuit the recorder refuses
    # (WP.PlanError: e.g. a decomposition range beyond 62 bits, a parameter beyond int64) has none and proves on the host path.
    try:
        plan = WP.record_plan(circuit).to_bytes()
    except WP.PlanError:
        plan = None
        if os.path.exists(pk_path + ".wplan"):                 # never leave another key's plan next to this one
            os.remove(pk_path + ".wplan")
    if plan is not None:
        open(pk_path + ".wplan", "wb").write(plan)
    return dict(n_advice=cs.n_advice, n_fixed=cs.n_fixed, n_lookups=len(cs.lookups), degree=cs.degree, pk_bytes=len(data))


def _rust_round(x):
    """f64::round: half away from zero (Python's round() is half to even)"""
    import math
    return int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))


def _quantize(v, scale, datum_type):
    """FileSourceInner::{as_type, to_field} (src/graph/input.rs:85-111) -> quantize_float (src/graph/utilities.rs:53-69): the value as the
    input's datum type would hold it (InputType::roundtrip, src/circuit/ops/mod.rs:112-141), times 2^scale, rounded half away from zero;
    values beyond what an i128 holds at that scale are the reference's SigBitTruncationError"""
    import struct
    if isinstance(v, bool):
        return 1 if v else 0
    if isinstance(v, str):                                   # a field element, as hex (FileSourceInner::Field)
        return codecs.felt_from_hex_le(v) % EL.R
    x = float(v)
    if datum_type == "F32":
        x = struct.unpack("f", struct.pack("f", x))[0]
    elif datum_type == "F16":                                # through half precision, as InputType::roundtrip does (f16::from_f64)
        x = float(np.float16(x))
    elif datum_type in ("Int", "TDim"):
        x = float(int(x))
    elif datum_type == "Bool":
        if int(x) not in (0, 1):
            raise ValueError("a Bool input must be 0 or 1")
        x = float(int(x))
    mult = 2.0 ** scale
    if abs(x) > round((2.0 ** 127 - 1) / mult):
        raise ValueError("SigBitTruncationError: the input does not fit the fixed-point representation")
    return _rust_round(mult * x)


def _phased(circuit):
    """whether the circuit's constraint system has advice beyond phase 0 (Freivalds einsums over its own configuration): its witness is
    made phase by phase, between the prover's commit stages, with the challenges squeezed so far"""
    return any(c.phase != 0 for c in circuit.gc.cs.advice)


def _first_phase(plan, x, columns=None):
    """what comes before the first commitment, on the device: phase 0 of the plan and the outputs, which live in it -> (columns,
    outputs).  A one-phase plan: its one-call run.  A plan with phases gathers its outputs with its LAST phase only, so they are taken
    by backend.WitnessPlan.outputs -- one more launch and one copy.  A witness the device refuses raises backend.WitnessError."""
    if plan.n_phases == 1:
        return plan.run(x, columns=columns)
    cols, _ = plan.run(x, columns=columns, phase=0)
    try:
        return cols, plan.outputs(cols)
    except BaseException:
        if columns is None:
            for c in cols:
                c.free()
        raise


def _host_advice(circuit, x, region=None):
    """the advice(phase, challenges) callable of native.create_proof and native.mock over the HOST layout of a phased circuit: phase 0 is
    `region` (the first-phase synthesis the caller already has, else made here), phase p > 0 the layout laid again with the challenges
    squeezed so far (ezkl_layout.host_phase_columns).  -> (the callable, columns: {column index: list of ints}, filled as the phases
    are asked for)"""
    per_phase, columns = EL.host_phase_columns(circuit, x, region), {}
    def advice(phase, challenges):
        cols = per_phase(phase, challenges)
        columns.update(cols)
        return dict(zip(cols, EL.cols_to_mont(list(cols.values()), B)))
    return advice, columns


def _module_result(points):
    """the ModuleForwardResult of one committed tensor as witness.json holds it, from PolyCommitChip::commit's affine Montgomery points"""
    out = []
    for p in points:
        xi, yi = (int.from_bytes(p[4 * h:4 * h + 4].tobytes(), "little") * pow(1 << 256, -1, B._Q) % B._Q for h in (0, 1))
        out.append({"x": codecs.felt_to_hex_le(xi), "y": codecs.felt_to_hex_le(yi)})
    return {"poseidon_hash": None, "polycommit": [out]}


def _forward_device(d, x, mode, pk_path, kzg=None):
    """gen_witness's forward pass on the device, for every family: the circuit's witness plan -- the `.wplan` next to pk_path where one is
    given and is this circuit's, else a fresh recording -- uploaded and replayed, the outputs read back, the lookup statistics by
    ezkl_hip_witness_lookup_stats_dev over the replayed cells.  Of a plan with phases only phase 0 is replayed (_first_phase): the
    outputs and every static lookup live in it, and a plan that has a nonlinearity record in a later phase is refused before the replay.  kzg (a resident backend.ParamsKZG, or None): the commitments of the circuit's KZG-committed tensors are then taken from the
    replayed module columns themselves (backend.polycommit_commit_dev: the tail rows filled with one, one table-free MSM over g_lagrange a
    column; the message never comes back to the host).  -> (outputs, (min, max), max_range_size, {tensor: points} or None), or None when mode is "auto" and
    the device path is not to be taken (_open_plan, or an input that does not fit int64); mode "device" raises instead.  A witness the
    device refuses raises backend.WitnessError, a ValueError with the layout's words."""
    if not _fits_plan(x, mode):
        return None
    circuit = _family(d["family"]).build(d)
    dev = _open_plan(circuit, pk_path, mode)
    if dev is None:
        return None
    cols = None
    try:
        late = [p for p in dev.lookup_phases if p > 0]
        if late:                                         # the statistics kernel reads the sources of every such record, in all phases
            raise ValueError("gen_witness: the plan has a nonlinearity record in phase %d; only phase 0 is replayed for a witness file" % late[0])
        cols, outs = _first_phase(dev, x)
        stats = dev.lookup_stats(cols)
        points = None
        if kzg is not None and callable(getattr(circuit, "committed", None)):          # last: it overwrites the unusable rows of those columns
            points = {what: B.polycommit_commit_dev([cols[blk[0].index] for blk in var.inner], length, POLYCOMMIT_BLINDING + 1, kzg)
                      for what, var, length in circuit.committed()}
    finally:
        for c in cols or []:
            c.free()
        dev.free()
    return [EL.signed(v) for v in outs], stats, _max_range_size(circuit), points


def gen_witness(compiled_circuit, data, output=None, vk_path=None, srs_path=None, synthesis="host", pk_path=None):
    """`ezkl gen-witness` (/root/reference/src/execute.rs:577-660 -> GraphCircuit::forward, src/graph/mod.rs:1734-1849; Python binding
    src/bindings/python.rs:914-941): the compiled circuit + the input data (GraphData JSON: a path, a JSON string or a dict with
    "input_data") -> the GraphWitness, written to `output` as the reference's witness.json and returned as a dict.

    * inputs are quantized as load_graph_input does (datum-type round trip, times 2^scale, half away from zero);
    * synthesis="host" (the default): the forward pass of the circuit's family (FAMILIES).  The MLP family's is the integer arithmetic of
      its ops (_mlp_of_graph: Einsum "mk,nk->mn", Add, LeakyReLU slope 0 at scale 0; a JSON description with "rebase" divides every Gemm's
      output by its layer's divisor, rounded half away from zero as the circuit's `div` claims it -- ezkl_layout.round_div -- and reports the
      outputs at the rebased scale) with the range checks the layout would make: a value outside (-base^legs, base^legs) where the
      circuit decomposes it is the reference's decomposition error, here a ValueError; max_range_size = decomp_base - 1.  The conv,
      pool_classifier and norm families run their circuit's own `synthesize`: the outputs are what it ties to the instance column,
      min_lookup_inputs / max_lookup_inputs what BaseRegion.nonlinearity kept of the signed inputs to every static lookup (both from 0, as
      region.rs:548-559 / graph/mod.rs:166-167), max_range_size the largest hi - lo of the circuit's range checks; a lookup input outside
      its table is a ValueError;
    * synthesis="device": the circuit's witness plan replayed on the GPU (the `.wplan` setup wrote next to pk_path, where pk_path is given,
      else a fresh recording), the statistics by the lookup-statistics kernel; raises where that cannot be done.  "auto": the device when
      the GPU gate is open and a device is there, else the host -- the rules of `prove`.  The witness.json bytes are the same either way;
    * KZGCommit visibility of the input / parameters / output ("polycommit", the MLP family only): PolyCommitChip::commit on the GPU (backend.polycommit_commit:
      one commit_lagrange MSM per column of 2^k - (blinding factors + 1) values) -- needs srs_path, and like the reference a vk to know the
      blinding factors (here: any file at vk_path; the count is read off the constraint system);  without an SRS the processed value stays
      None, as in the reference ("SRS for poly commit does not exist (will be ignored)").  On the host path the message is the tensor
      as Python integers (the parameters in the order the circuit's module holds them: per layer the weight rows, then the bias --
      MlpCircuit.flat_params); on the device path it is the replayed module column itself (_forward_device).  Either way a tensor of
      `len` values gets len // n + 1 commitments, n = 2^k - 6, as the reference computes it: when len is a multiple of n the last one is the
      commitment to an EMPTY column (zeros and the six ones) -- which the circuit has too, VarTensor.new_advice leaves room for a
      duplicated row that a module never writes.  (For other lengths the circuit can have one column MORE than the file has
      commitments, e.g. len = n - 1: the reference's swap-proof-commitments then misplaces every later tensor's points; so does ours.)
      Hashed (Poseidon) visibility, a Fixed input or output and a Private output are refused by name."""
    if synthesis not in ("auto", "host", "device"):
        raise ValueError("synthesis must be \"auto\", \"host\" or \"device\"")
    d, _ = _read_compiled(compiled_circuit, any_visibility=True)
    ra, vis, in_scale, out_scale = d["run_args"], d["visibility"], d["in_scale"], d["out_scale"]
    for what, v in vis.items():
        if isinstance(v, dict):
            raise ValueError("unsupported visibility: %s is Hashed (Poseidon modules are outside this package's scope)" % what)
    if d["family"] == "mlp":
        EL.visibility_triple(vis)
    if isinstance(data, (bytes, str)) and os.path.exists(data):
        data = open(data).read()
    if isinstance(data, (bytes, str)):
        data = json.loads(data)
    cols = data["input_data"]
    if len(cols) != 1 or len(cols[0]) != d["n_inputs"]:
        raise ValueError("input data does not match the circuit's input shape")
    x = [_quantize(v, in_scale, d["datum_type"]) for v in cols[0]]
    x = [EL.signed(v % EL.R) for v in x]
    inputs = list(x)
    processed = dict(input=None, params=None, output=None)
    committed = [what for what in ("input", "params", "output") if vis[what] == "KZGCommit"]
    kzg = None
    if committed and vk_path is not None and srs_path is not None and os.path.exists(srs_path):
        srs = load_params_prover(srs_path, ra["logrows"])
        bg = _srs_bases(srs["g"], "g")
        try:
            bgl = _srs_bases(srs["g_lagrange"], "g_lagrange")
        except BaseException:
            bg.free()
            raise
        kzg = B.ParamsKZG.from_bases(ra["logrows"], bg, bgl)
    try:
        made = _forward_device(d, x, synthesis, pk_path, kzg) if synthesis != "host" else None
        if made is not None:
            outputs, (min_lookup, max_lookup), max_range_size, points = made
        else:
            (outputs, (min_lookup, max_lookup), max_range_size), points = _family(d["family"]).forward(d, x), None
        if kzg is not None and points is None:               # the host path: PolyCommitChip::commit of the message as integers
            weights, biases = d.get("weights"), d.get("biases")                     # (what a KZGCommit of the parameters commits to: the MLP family's)
            messages = dict(input=inputs, output=outputs, params=[v for W, bv in zip(weights, biases) for v in [w for row in W for w in row] + list(bv)])
            def commit(vals):
                msg = np.stack([np.frombuffer(((v % EL.R) * (1 << 256) % EL.R).to_bytes(32, "little"), np.uint64) for v in vals])
                return B.polycommit_commit(msg, POLYCOMMIT_BLINDING + 1, kzg, once=True)    # the SRS is loaded for these one to three columns
            points = {what: commit(messages[what]) for what in committed if messages[what]}
        for what in committed:
            if kzg is None:                                  # the reference: a module result without its commitments
                processed[what] = {"poseidon_hash": None, "polycommit": None}
            elif what in points:
                processed[what] = _module_result(points[what])
    finally:
        if kzg is not None:
            kzg.free()
    text = codecs.write_witness_json([[v % EL.R for v in inputs]], [[v % EL.R for v in outputs]], [in_scale], [out_scale],
                                     processed_inputs=processed["input"], processed_params=processed["params"], processed_outputs=processed["output"],
                                     max_lookup_inputs=max_lookup, min_lookup_inputs=min_lookup, max_range_size=max_range_size)
    if output is not None:
        open(output, "w").write(text)
    return json.loads(text)


def _plan_for(circuit, pk_path):
    """the witness plan setup wrote next to the key, if it is THIS circuit's (geometry and parameter hash); otherwise -- or without a key
    path -- a fresh recording"""
    try:
        if pk_path is None:
            raise OSError("no key path")
        blob = open(pk_path + ".wplan", "rb").read()
        h = WP.peek(blob)
        if (h["k"], h["n_advice"], h["n_inputs"], h["param_hash"]) == (circuit.k, len(circuit.gc.cs.advice), circuit.n_inputs, WP.params_hash(circuit)):
            return blob                                   # the upload validates the rest
    except (OSError, WP.PlanError):
        pass
    return WP.record_plan(circuit).to_bytes()


def _fits_plan(x, mode):
    """whether the plan's int64 lanes hold the inputs x; mode "device" raises where they do not ("auto" then takes the host layout)"""
    fits = all(-(1 << 63) <= v < 1 << 63 for v in x)
    if not fits and mode == "device":
        raise ValueError("synthesis=\"device\": an input does not fit int64")
    return fits


def _read_witness(circuit, witness_path, synthesis, parsed=None):
    """the GraphWitness file checked against the circuit, before anything is loaded for it: -> (the parsed file, the inputs as signed
    integers).  synthesis "device" refuses here an input the plan's int64 lanes cannot hold."""
    w = parsed if parsed is not None else codecs.read_witness_json(open(witness_path).read())
    if len(w["inputs"]) != 1 or len(w["inputs"][0]) != circuit.n_inputs:
        raise ValueError("witness does not match the circuit's input shape")
    x = [EL.signed(v) for v in w["inputs"][0]]
    _fits_plan(x, synthesis)
    return w, x


def _open_plan(circuit, pk_path, mode):
    """the witness plan on the device (backend.WitnessPlan), validated and uploaded, or None when mode is "auto" and the device path
    is not to be taken: the gate is closed (ezkl_amd.enabled), there is no device, or the recorder refuses the circuit (WP.PlanError).
    mode "device" raises instead."""
    import ezkl_amd
    forced = mode == "device"
    if not forced and not ezkl_amd.enabled(circuit.k):
        return None
    if len(circuit.gc.cs.advice) > 64:
        if forced:
            raise ValueError("synthesis=\"device\": the circuit has more than 64 advice columns")
        return None
    try:
        blob = _plan_for(circuit, pk_path)
    except WP.PlanError:                                 # a circuit the host engine lays out and the recorder does not: the host path
        if forced:
            raise
        return None
    try:
        return B.WitnessPlan(blob)
    except ezkl_amd.EzklHipError as e:
        if forced or e.code != -1:                       # EZKL_ERR_NO_DEVICE: the host path, as before
            raise
        return None


def _device_witness(circuit, pk_path, x, mode):
    """one synthesis on the device outside a session: -> (resident advice columns, instance column, the run's counters), or None when
    mode is "auto" and the device path is not to be taken (_open_plan, or an input that does not fit int64).  mode "device" raises
    instead."""
    if not _fits_plan(x, mode):
        return None
    dev = _open_plan(circuit, pk_path, mode)
    if dev is None:
        return None
    try:
        cols, outs = dev.run(x)
        return cols, circuit.instances(x, outs), dev.last
    finally:
        dev.free()


class Prover:
    """A proving session: everything `prove` needs that does not depend on the witness is loaded ONCE and stays resident until close() --
    the circuit and its constraint system (rebuilt from the key's selector rows, _plonk_cs), the proving key (NativeProvingKey.from_file),
    both base sets (an SRS file larger than the circuit is downsized on the device and the two sets downsize returns are kept as they
    are), g2 / s_g2, and -- where the witness is made on the device -- the witness plan with ONE set of advice columns that every proof
    writes again.  A proof is then the plan's replay plus create_proof.

        with Prover(compiled_circuit, pk_path, srs_path) as p:
            for w in witness_files:
                proof = p.prove(w, w + ".proof.json")

    recommit / synthesis: as for `prove` below (the plan rules are the same: "host" opens no plan, "device" raises where the plan cannot
    be had, "auto" takes it when the GPU gate is open and falls back to the host layout otherwise).
    .opened: the load stages and their wall seconds.  A witness the device refuses (backend.WitnessError) or whose outputs disagree with
    the circuit's raises and leaves the session as it was: the next prove() runs on the same buffers."""

    def __init__(self, compiled_circuit, pk_path, srs_path, recommit=False, synthesis="auto", _circuit=None):
        import time
        if synthesis not in ("auto", "host", "device"):
            raise ValueError("synthesis must be \"auto\", \"host\" or \"device\"")
        self.synthesis, self.opened = synthesis, {}
        self.circuit = self.native = self.pk = self.bg = self.bgl = self.plan = self.g2 = self.s_g2 = None
        self._cols, self._open = [], False
        def stage(name, t0):
            self.opened[name] = self.opened.get(name, 0.0) + time.perf_counter() - t0
            return time.perf_counter()
        try:
            t = time.perf_counter()
            self.circuit = _circuit if _circuit is not None else _load_circuit(compiled_circuit)[0]      # (`prove` has loaded it already)
            t = stage("circuit", t)
            self.native = NV.NativeCircuit(_plonk_cs(self.circuit, pk_path))
            t = stage("constraint_system", t)
            k = self.circuit.k
            srs = _read_srs(srs_path, k)
            self.g2, self.s_g2 = srs["g2"], srs["s_g2"]
            t = stage("srs_read", t)
            if srs["k"] > k:                                     # load_params_prover's downsize, its two resident sets kept
                self.bg, self.bgl = _downsized(srs, k)
            else:
                self.bg = _srs_bases(srs["g"], "g")
                self.bgl = _srs_bases(srs["g_lagrange"], "g_lagrange")
            del srs
            self.bg.prepare(); self.bgl.prepare()                # the window tables build while the key is read
            t = stage("srs_to_device", t)
            # recommit: the key file's commitments were made under ANOTHER SRS (the reference's fixture key: the public powers of tau)
            self.pk = NV.NativeProvingKey.from_file(self.native, pk_path, recommit=self.bg if recommit else None)
            t = stage("key", t)
            if synthesis != "host":
                self.plan = _open_plan(self.circuit, pk_path, synthesis)
                if self.plan is not None:
                    for _ in range(self.plan.n_advice):
                        self._cols.append(B.DeviceBuffer(32 << self.plan.k))
            t = stage("plan", t)
        except BaseException:
            self._free()
            raise
        self._open = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _free(self):
        for c in self._cols:
            c.free()
        self._cols = []
        for name in ("plan", "pk", "bg", "bgl", "native"):
            h = getattr(self, name)
            if h is not None:
                h.free()
            setattr(self, name, None)
        self.circuit = self.g2 = self.s_g2 = None

    def close(self):
        """free everything the session holds (device and host); a later prove() raises.  Closing twice is harmless."""
        self._open = False
        self._free()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def prove(self, witness_path, proof_path=None, check_mode=CheckMode.UNSAFE, seed=0, report=None, _witness=None):
        """one proof of this session's circuit: GraphWitness file -> proof bytes (written as proof.json to proof_path when one is given).
        seed, check_mode and what report receives are `prove`'s below; report["stages"] adds the wall seconds of each stage of this call
        (witness_read, synthesis, [host_columns,] create_proof, [proof_write]) and report["create_proof_breakdown"] the prover's own
        split of create_proof.  A circuit with second-phase advice (_phased) is proved through a callable: "synthesis" is then its first
        phase and the outputs, the later phases run inside create_proof -- on the device by the plan's replay with the prover's
        challenges, report["phase_ms"] = {phase: device milliseconds}; with synthesis="host" by the layout laid again."""
        import time
        if not self._open:
            raise RuntimeError("this Prover is closed")
        stages = {}
        t = time.perf_counter()
        def stage(name):
            nonlocal t
            now = time.perf_counter()
            stages[name] = now - t
            t = now
        circuit = self.circuit
        w, x = _witness if _witness is not None else _read_witness(circuit, witness_path, self.synthesis)      # (`prove` has read it already)
        stage("witness_read")
        on_device = self.plan is not None and _fits_plan(x, self.synthesis)                 # "auto": wider inputs take the host layout
        phased, advice, resident = _phased(circuit), None, ()
        if on_device:
            _, outs = _first_phase(self.plan, x, columns=self._cols)            # into the session's columns, whatever they held
            adv, inst = self._cols, circuit.instances(x, outs)
            how = dict(self.plan.last, path="device")
            if phased:                                                          # the columns of phase 0 as they are; phase p > 0 replayed with the prover's challenges
                plan, cols, phase_ms = self.plan, self._cols, {0: self.plan.last["device_ms"]}
                how["phase_ms"] = phase_ms
                def advice(phase, challenges):
                    if phase > 0:
                        plan.run(x, columns=cols, phase=phase, challenges=list(challenges))
                        phase_ms[phase] = plan.last["device_ms"]
                    return {c: cols[c] for c in range(plan.n_advice) if plan.column_phase[c] == phase}
                resident = range(plan.n_advice)
        elif phased:
            reg = circuit.synthesize(x, True)                                   # the first phase: the outputs live in it
            inst, how = [list(circuit.outputs)], dict(path="host")
            advice, _ = _host_advice(circuit, x, reg)
        else:
            adv, inst = circuit.witness(x)                                      # GraphCircuit::synthesize
            how = dict(path="host")
        stage("synthesis")
        if report is not None:
            report.clear()
            report.update(how)
            report["stages"] = stages
        if w["outputs"] and [list(outs if on_device else circuit.outputs)] != w["outputs"]:
            raise ValueError("the witness file's outputs do not match the circuit's outputs")
        if not on_device and not phased:
            adv = EL.cols_to_mont(adv, B)
            stage("host_columns")
        tm = {}
        proof = NV.create_proof(self.pk, self.bg, self.bgl, advice if phased else adv, seed=seed, instances=inst, check_mode=check_mode, g2=self.g2,
                                s_g2=self.s_g2, timings=tm, device_columns=resident)
        stage("create_proof")
        if report is not None:
            report["create_proof_breakdown"] = tm
        if proof_path is not None:
            open(proof_path, "w").write(codecs.write_proof_json(proof, inst))
            stage("proof_write")
        return proof


def prove(witness_path, compiled_circuit, pk_path, proof_path, srs_path, check_mode=CheckMode.UNSAFE, seed=0, recommit=False, synthesis="auto",
          report=None):
    """GraphWitness + compiled circuit + pk + SRS files -> proof.json (Snark).  seed = 0: OS entropy (OsRng); otherwise the
    reference's det-prove.  CheckMode.SAFE verifies the proof before returning it, as create_proof_circuit does.
    synthesis: where the advice columns are made -- "host": the layout engine, cell by cell (circuit.witness), uploaded by create_proof;
    "device": the witness plan replayed by HIP kernels into resident columns that create_proof takes as they are (raises if that cannot
    be done); "auto": the device when the GPU gate is open (ezkl_amd.enabled(k)) and a device is there, else the host.  The proof bytes
    are the same either way.  report (a dict, may be None) receives how the witness was made: {"path": "host"} or {"path": "device",
    "cells_written", "launches", "device_ms", ...} -- the counters of backend.WitnessPlan.run.
    One proof per call: a Prover session opened, used once and closed.  Whoever proves more than once keeps the Prover."""
    if synthesis not in ("auto", "host", "device"):
        raise ValueError("synthesis must be \"auto\", \"host\" or \"device\"")
    # the witness is read and checked against the circuit first, as ever: a file that does not fit is refused before the SRS, the key
    # and the plan are loaded for it
    parsed = codecs.read_witness_json(open(witness_path).read())
    circuit, _ = _load_circuit(compiled_circuit)
    witness = _read_witness(circuit, witness_path, synthesis, parsed)
    how = {} if report is not None else None
    try:
        with Prover(compiled_circuit, pk_path, srs_path, recommit=recommit, synthesis=synthesis, _circuit=circuit) as session:
            return session.prove(witness_path, proof_path, check_mode=check_mode, seed=seed, report=how, _witness=witness)
    finally:
        if how:                                                                 # what it always held, from the moment the witness is made; the
            report.clear()                                                      # session's timings stay with the session
            report.update({a: b for a, b in how.items() if a not in ("stages", "create_proof_breakdown")})


def verify(proof_path, compiled_circuit, vk_path=None, srs_path=None, recommit=False, pk_path=None):
    """-> True / False, from the proof, the compiled circuit (settings), vk.key and the SRS's g2 / s_g2 -- what the reference's `verify`
    reads (src/execute.rs:1651).  Host only: no GPU, no proving key, none of the prover's private weights, and no layout of the circuit:
    the constraint system is rebuilt from the key's own selector rows (_plonk_cs).  A pk.key path works too (vk.key is its prefix, and only
    that prefix is read).  recommit=True (a key whose commitments were made under another SRS, re-committed by `prove`) needs the proving
    key and a device: the fixed / permutation polynomials are committed again under this SRS first."""
    if vk_path is None:
        vk_path = pk_path                                                       # the parameter's former name: keyword callers keep working
    if vk_path is None or srs_path is None:
        raise TypeError("verify needs a vk.key (or pk.key) path and an SRS path")
    circuit, j = _load_circuit(compiled_circuit)
    pr = codecs.read_proof_json(open(proof_path).read())
    cs_, vk_bytes = _key_system(circuit, vk_path)
    if not recommit:
        g2, s_g2 = codecs.read_srs_g2(srs_path)
        return NV.verify_proof_vk(NV.NativeCircuit(cs_), vk_bytes, g2, s_g2, pr["proof"], pr["instances"])
    # len(vk_bytes) is the exact length of a vk.key of this constraint system (codecs.py): header, the fixed + permutation commitments AND
    # the bit-packed selector rows (80 selectors at k = 20 are 10 MB: ADVICE r04 -- a bound without them let a vk-only file through to a
    # later, misleading "proving key truncated")
    if os.path.getsize(vk_path) <= len(vk_bytes):                               # a vk-only file has no polynomials to commit again
        raise ValueError("recommit=True needs the PROVING key file (its polynomials are committed again under this SRS); %s is a verifying key" % vk_path)
    srs = codecs.read_srs(open(srs_path, "rb").read())
    bg = _srs_bases(srs["g"], "g")
    try:
        pk = NV.NativeProvingKey.from_file(NV.NativeCircuit(cs_), vk_path, recommit=bg)
        return NV.verify_proof(pk, srs["g2"], srs["s_g2"], pr["proof"], pr["instances"])
    finally:
        bg.free()


def witness_commitments(witness):
    """GraphWitness::get_polycommitments: the KZG commitments of a witness file (a path, or the parsed JSON) as (x, y) integers, in the
    order input, params, output -- the order of the module columns, which are the first advice columns of the circuit"""
    w = json.load(open(witness)) if isinstance(witness, (str, bytes, os.PathLike)) else witness
    return [(codecs.felt_from_hex_le(p["x"]), codecs.felt_from_hex_le(p["y"]))
            for key in ("processed_inputs", "processed_params", "processed_outputs")
            for group in ((w.get(key) or {}).get("polycommit") or []) for p in group]


def swap_proof_commitments(proof_path, witness_path):
    """`ezkl swap-proof-commitments` (src/execute.rs:1629-1650 of the reference -> pfsys::swap_proof_commitments, src/pfsys/mod.rs:492-554):
    the witness file's KZG commitments, in the order input, params, output, written as the EVM transcript writes points (32 bytes
    big-endian x, then y) over the FIRST bytes of the proof -- the commitments to the module columns are the first points of a proof --,
    the hex form refreshed, the file saved in place.  A proof made from that witness is left as it is; one made from another input or
    other parameters no longer verifies.  A witness without commitments changes nothing, and the result says so.
    -> dict(commitments: how many were written, changed: whether the proof bytes differ now, proof: the bytes, note)"""
    points = witness_commitments(witness_path)
    j = json.loads(open(proof_path).read())
    old = codecs.read_proof_json(json.dumps(j))["proof"]
    head = b"".join(c.to_bytes(32, "big") for p in points for c in p)
    if len(head) > len(old):
        raise ValueError("the witness holds %d commitments, the proof only %d bytes" % (len(points), len(old)))
    new = head + old[len(head):]
    j["proof"], j["hex_proof"] = list(new), "0x" + new.hex()                     # create_hex_proof
    open(proof_path, "w").write(json.dumps(j, separators=(",", ":")))
    note = "no commitments found in witness: the proof is unchanged" if not points else \
           ("swap proof has created a different proof" if new != old else "the proof already carried these commitments")
    return dict(commitments=len(points), changed=new != old, proof=new, note=note)


def _key_system(circuit, key):
    """(the constraint system as keygen saw it, the key's vk.key bytes), WITHOUT laying the circuit out: halo2's key file carries every
    selector's rows bit-packed (vk.key, which pk.key starts with), and `configure` + selector compression on those rows is what halo2 itself
    does on load_pk (src/pfsys/mod.rs:627).  key: a path or the bytes.  Of a file only the vk prefix is read -- a pk.key is GiBs at k = 20.
    The permutation-column and selector counts are the configured system's, the fixed-column count is the file's; a key whose header or
    whose count of fixed columns after compression says it was made for another circuit is a ValueError, one too short for its
    selector section the loader's own RuntimeError."""
    import struct
    cs0 = circuit.fresh().gc.cs                                                 # compress_selectors rewrites the system in place: a fresh one
    n_perm, n_sel = len(cs0.permutation), len(cs0.selectors)
    def vk_len(head):
        if len(head) < 7:
            raise RuntimeError("verifying key truncated: %d bytes" % len(head))
        if head[0] != 3:
            raise ValueError("unsupported key version %d" % head[0])
        if head[1] != circuit.k:
            raise ValueError("the key does not belong to this circuit: it was made for k = %d, the circuit has k = %d" % (head[1], circuit.k))
        return 7 + 64 * (struct.unpack_from("<I", head, 3)[0] + n_perm) + n_sel * (((1 << circuit.k) + 7) // 8)
    if isinstance(key, (bytes, bytearray, memoryview)):
        want = vk_len(bytes(key[:7]))
        raw = bytes(key[:want])
    else:
        with open(key, "rb") as f:
            head = f.read(7)
            want = vk_len(head)
            raw = head + f.read(want - 7)
    if len(raw) < want:
        raise RuntimeError("verifying key truncated (selector section): %d bytes of %d" % (len(raw), want))
    vk = codecs.read_vk(raw, n_perm, n_sel)
    cs0.compress_selectors(list(vk["selectors"]))
    cs = cs0.to_plonk(circuit.k)
    if cs.n_fixed != vk["fixed_commitments"].shape[0]:
        raise ValueError("the key does not belong to this circuit: it commits to %d fixed columns, the circuit's selector rows in it compress to %d"
                         % (vk["fixed_commitments"].shape[0], cs.n_fixed))
    return cs, raw


def _plonk_cs(circuit, key=None):
    """the constraint system as keygen saw it, from the key (a path or bytes) and the configured circuit: see _key_system.  Without a
    key (`mock` has none) the selector activations come from a fresh layout pass, as long as the host synthesis is."""
    if key is None:
        return _fresh_keygen_inputs(circuit)[0]
    return _key_system(circuit, key)[0]


def _fresh_keygen_inputs(circuit):
    """(cs, fixed, copies, region) of a fresh synthesis pass without witness values: what keygen saw (`mock`, which has no key)"""
    return circuit.fresh().keygen_inputs([0] * circuit.n_inputs)


class MockError(ValueError):
    """`mock` found unsatisfied constraints: .records = [(kind, index, sub, row)] (kind 1 gate, 2 lookup, 3 copy; at most the first
    MOCK_CAP, sorted), .totals = exact failure counts (gates, lookups, copies)"""

    def __init__(self, msg, records, totals):
        super().__init__(msg)
        self.records, self.totals = records, totals


MOCK_CAP = 1024
_KIND_NAMES = {"adv": "advice", "fix": "fixed", "inst": "instance"}


def mock(witness_path, compiled_circuit):
    """`ezkl mock` (/root/reference/src/execute.rs:1280-1305: MockProver::run(logrows, &circuit, public_inputs).verify()) on the GPU: the
    witness is laid out by the synthesis `prove` uses and every gate, lookup and copy constraint is checked row by row
    (native.mock -> ezkl_prover_mock).  No SRS, no keys.  The public inputs are the witness file's outputs (prepare_public_inputs), so a
    wrong output is a failing copy into the instance column.  A circuit with second-phase advice is laid out once per phase, at the challenges
    the mock prover draws (_host_advice).  Returns "" when every constraint holds; raises MockError otherwise, its message
    naming the first failures (gate / row, lookup / input / row, the two cells of a copy)."""
    w = codecs.read_witness_json(open(witness_path).read())
    circuit, j = _load_circuit(compiled_circuit)
    w, x = _read_witness(circuit, witness_path, "host", w)
    if _phased(circuit):                                                        # one layout pass per phase, at the challenges the mock prover draws
        advice, by_index = _host_advice(circuit, x)
        advice(0, [])                                                           # the first phase, kept for the mock prover's call: the outputs live in it
        adv, inst = None, [list(circuit.outputs)]
    else:
        adv, inst = circuit.witness(x)                                          # GraphCircuit::synthesize
    cs, fixed, copies, _ = _fresh_keygen_inputs(circuit)
    public = circuit.instances(x, w["outputs"][0]) if w["outputs"] else inst     # prepare_public_inputs: from the witness file
    records, totals = NV.mock(cs, EL.cols_to_mont(fixed, B), copies, advice if adv is None else EL.cols_to_mont(adv, B), instances=public, seed=1,
                              cap=MOCK_CAP)
    if adv is None:
        adv = [by_index.get(c) or [0] * cs.n for c in range(cs.n_advice)]
    if not any(totals):
        return ""
    cols = {"adv": adv, "fix": fixed, "inst": [list(c) + [0] * (cs.n - len(c)) for c in public]}
    value = lambda cell: int(cols[cs.perm[cell[0]][0]][cs.perm[cell[0]][1]][cell[1]]) % EL.R
    name = lambda cell: "%s %d, row %d" % (_KIND_NAMES[cs.perm[cell[0]][0]], cs.perm[cell[0]][1], cell[1])
    cycles = None
    lines = []
    for kind, index, sub, row in records[:10]:
        if kind == 1:
            lines.append("gate %d not satisfied on row %d" % (index, row))
        elif kind == 2:
            lines.append("lookup %d input %d row %d: not in table" % (index, sub, row))
        else:
            if cycles is None:                                                  # the copy cycles, for naming the cell a failing one differs from
                parent = {}
                def find(x):
                    while parent.setdefault(x, x) != x:
                        parent[x] = parent[parent[x]]
                        x = parent[x]
                    return x
                for a, b in copies:
                    parent[find(tuple(a))] = find(tuple(b))
                cycles = {}
                for x in list(parent):
                    cycles.setdefault(find(x), []).append(x)
                cycles = {x: members for members in cycles.values() for x in members}
            cell = (index, row)
            other = next((o for o in sorted(cycles.get(cell, [])) if value(o) != value(cell)), None)
            lines.append("copy (%s) != (%s)" % (name(cell), name(other)) if other else "copy (%s) differs from its copy cycle" % name(cell))
    msg = "mock: %d gate, %d lookup and %d copy constraint failures: %s" % (totals[0], totals[1], totals[2], "; ".join(lines))
    raise MockError(msg, records, totals)
