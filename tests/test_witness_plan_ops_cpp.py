"""The C++ parser's scan, gather and clamp rules (ezkl_amd/csrc/witness_plan.hpp) as a plain program under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/cpp/test_witness_plan_ops.cpp reads the blobs written here -- synthetic plans of the new kinds it must
take, and every plan of witness_synth_ops.bad_plans() with the message the Python validator gave for it -- and says what it asserts.  No
device, no library loaded into the interpreter, no preload."""
import witness_synth_ops as O
import wplan_cpp

GOOD = ["sum-ragged-33-17-16-5-1-w3", "prod-partial-operandless-ragged", "sum-scans9-steps33-w3", "prod-special-values", "gather-lanes257-table300",
        "gather-outside-table1-lanes65", "clamp-bounds-and-edges"]


def test_the_parser_additions_under_the_sanitizers(tmp_path):
    plans = [O.small_plan().plan] + [O.CASES[name](1).plan for name in GOOD]
    wplan_cpp.parser_program(tmp_path, "test_witness_plan_ops", plans, O.bad_plans(), ends_with=False)
