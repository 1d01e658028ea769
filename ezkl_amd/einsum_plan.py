"""The Freivalds einsum's planning, restated: which reductions `Einsums::assign_einsum` lays out for an equation, in which order and in
which phase, and how many rows of the einsum columns they take.

  einsum_reductions   reduction_planner::input_reductions   /root/reference/src/circuit/ops/chip/einsum/reduction_planner.rs:85-205
  einsum_analysis     analysis::analyze_single_equation     /root/reference/src/circuit/ops/chip/einsum/analysis.rs:84-209

Plain data, no layout: ezkl_layout.EinsumCircuit walks the plan.  The details that decide the layout are the reference's: the output axes
are walked in equation order, the axes that remain in sorted order (a BTreeSet), a result's expression is the sorted set of its
characters, `retain` drops every tensor whose expression STRING was consumed, and an RLC's challenge is the axis's position in the output
expression."""
import collections
import math

RLC = collections.namedtuple("RLC", "expression axis input_index input_phase challenge_index")
Contraction = collections.namedtuple("Contraction", "expression axis input_indices input_phases output_phase")   # axis None: a pairwise product
Analysis = collections.namedtuple("Analysis", "equation output_indices num_output_axes reduction_length strategy num_inputs max_input_size output_size")
BASE_OPS, FREIVALDS = "BaseOps", "Freivalds"


def reduction_inputs(red):
    """Reduction::input_indices (reduction_planner.rs:70-75)"""
    return [red.input_index] if isinstance(red, RLC) else list(red.input_indices)


def reduction_output_phase(red):
    """Reduction::output_phase (:77-82): an RLC's result is always second-phase"""
    return 1 if isinstance(red, RLC) else red.output_phase


def einsum_reductions(equation):
    """input_reductions (reduction_planner.rs:85-205): the ordered reductions that squash the operands of `equation` to scalars.  Tensor i
    of the plan is operand i for i < the number of operands, then the result of reduction i - that number."""
    input_exprs, output_expr = equation.split("->")
    exprs = [((0, e), i) for i, e in enumerate(input_exprs.split(","))]          # ((phase, expression), tensor index)
    counter = len(exprs)
    reductions = []

    def reduce(exprs, axis):                                                       # :100-175
        nonlocal counter
        inputs = [x for x in exprs if axis in x[0][1]]
        phases, axes, indices = [p for (p, _), _ in inputs], [e for (_, e), _ in inputs], [i for _, i in inputs]
        is_output_axis = axis in output_expr
        if is_output_axis and len(inputs) > 1:
            output = "".join(sorted(set("".join(axes))))
        else:
            output = "".join(sorted(set(c for e in axes for c in e if c != axis)))
        if is_output_axis and len(inputs) == 1:
            red = RLC("%s,%s->%s" % (",".join(axes), axis, output), axis, indices[0], phases[0], output_expr.index(axis))
        else:
            red = Contraction("%s->%s" % (",".join(axes), output), None if is_output_axis else axis, indices, phases, max(phases))
        exprs = [x for x in exprs if x[0][1] not in axes]                          # `retain`: by expression string
        exprs.append(((reduction_output_phase(red), output), counter))
        counter += 1
        return red, exprs

    output_axes = list(output_expr)
    while output_axes:                                                             # :177-190
        axis = output_axes[0]
        if not any(axis in e for (_, e), _ in exprs):
            output_axes.pop(0)
        else:
            red, exprs = reduce(exprs, axis)
            reductions.append(red)
    for axis in sorted(set(c for (_, e), _ in exprs for c in e)):                  # :193-202 (the set is taken once, before the loop)
        red, exprs = reduce(exprs, axis)
        reductions.append(red)
    return reductions


def sanitised(equation, dims):
    """the equation without its axes of extent 1 (analysis.rs:89-111); dims: axis -> extent for every axis of an operand"""
    inputs_str, output_str = equation.split("->")
    inputs = ["".join(c for c in e if dims[c] > 1) for e in inputs_str.split(",")]
    return ",".join(inputs) + "->" + "".join(c for c in output_str if dims.get(c, 0) > 1)


def einsum_analysis(equation, dims):
    """analyze_single_equation (analysis.rs:84-209)"""
    equation = sanitised(equation, dims)
    inputs_eq, output_eq = equation.split("->")
    input_equations = inputs_eq.split(",")
    max_input_size = max(math.prod(dims[c] for c in e) for e in input_equations)
    output_indices = list(output_eq)
    output_dims = [dims[c] for c in output_indices]
    rest, output_reduction = output_dims[::-1], 0                                  # :132-141: the axes from the last one on
    while rest:
        length = rest.pop(0)
        output_reduction += length * math.prod(rest)
    input_reduction = 0
    for red in einsum_reductions(equation):                                        # :143-168
        out = red.expression.split("->")[1]
        length = dims[red.axis] if red.axis is not None else 1
        n_inputs = len(reduction_inputs(red))
        input_reduction += math.prod(dims[c] for c in out) * (length if n_inputs <= 2 else length * n_inputs)
    seen, common = set(), []                                                       # :170-192
    for e in input_equations:
        for c in e:
            if c in seen:
                common.append(c)
            seen.add(c)
    non_common = [c for c in dims if c not in common and dims[c] > 1]
    base_ops = not (len(output_indices) > 0 and len(common) > 0 and len(non_common) > 1)
    return Analysis(equation, output_indices, len(output_indices), output_reduction + input_reduction, BASE_OPS if base_ops else FREIVALDS,
                    len(input_equations), max_input_size, math.prod(output_dims))
