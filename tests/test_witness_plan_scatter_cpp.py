"""The C++ parser's SCATTER, COMPLEMENT and ONEHOT rules (ezkl_amd/csrc/witness_plan.hpp) as a plain program under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/cpp/test_witness_plan_scatter.cpp reads the blobs written here -- synthetic plans of the new kinds it must
take, the plan recorded from a ScatterGatherCircuit, and every plan of witness_synth_scatter.bad_plans() with the message the Python
validator gave for it -- and says what it asserts.  No device, no library loaded into the interpreter, no preload."""
import witness_synth_scatter as T
import wplan_cpp

GOOD = ["scatter-n1", "scatter-n2", "scatter-n65", "scatter-n257", "complement-n1", "complement-n2", "complement-n64", "complement-n257", "onehot-edges", "onehot-outside"]


def test_the_indexed_rules_of_the_parser_under_the_sanitizers(tmp_path):
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    recorded = [WP.record_plan(EL.ScatterGatherCircuit(10, 2, 6000))]
    plans = ([T.small_plan().plan, T.failing_case(100, True).plan, T.failing_case(T.TILE + 1, True).plan, T.CASES["complement-n%d" % (T.TILE + 1)](1).plan] + recorded +
             [T.CASES[name](1).plan for name in GOOD])
    wplan_cpp.parser_program(tmp_path, "test_witness_plan_scatter", plans, T.bad_plans())
