"""The C++ parser's SORT / ARGSORT rules (ezkl_amd/csrc/witness_plan.hpp) as a plain program under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/cpp/test_witness_plan_sort.cpp reads the blobs written here -- synthetic plans of the new kinds it must
take, the plan recorded from a SortTopkCircuit, and every plan of witness_synth_sort.bad_plans() with the message the Python validator
gave for it -- and says what it asserts.  No device, no library loaded into the interpreter, no preload."""
import witness_synth_sort as T
import wplan_cpp

GOOD = ["sort-n1-mode0", "sort-n65-mode1", "sort-n2049-mode0", "sort-single-n3-mode1", "sort-9x100-mode1", "sort-300x5-mode0"]


def test_the_sort_rules_of_the_parser_under_the_sanitizers(tmp_path):
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    recorded = WP.record_plan(EL.SortTopkCircuit(9, 2, 3000, 8, 3, True, "largest_index_first", 16, 2))
    plans = [T.small_plan().plan, T.failing_case(100, True).plan, recorded] + [T.CASES[name](1).plan for name in GOOD]
    wplan_cpp.parser_program(tmp_path, "test_witness_plan_sort", plans, T.bad_plans(), ends_with=False)
