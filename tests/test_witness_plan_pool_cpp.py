"""The C++ parser's ARGEXT rules (ezkl_amd/csrc/witness_plan.hpp) as a plain program under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/cpp/test_witness_plan_pool.cpp reads the blobs written here -- synthetic plans of the new kind it must
take, the plans recorded from a PoolClassifierCircuit (max and sum pooling), and every plan of witness_synth_pool.bad_plans() with the
message the Python validator gave for it -- and says what it asserts.  No device, no library loaded into the interpreter, no preload."""
import witness_synth_pool as T
import wplan_cpp

GOOD = ["argext-n1-mode0", "argext-n3-mode1", "argext-n64-mode0", "argext-n65-mode1", "argext-n257-mode0", "argext-300x5-mode1", "argext-130x1-mode0"]


def test_the_arg_extremum_rules_of_the_parser_under_the_sanitizers(tmp_path):
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    recorded = [WP.record_plan(EL.PoolClassifierCircuit(10, 2, 12000, pool=pool)) for pool in ("max", "sum")]
    plans = [T.small_plan().plan, T.failing_case(100, True).plan, T.failing_case(T.CHUNK + 1, True).plan] + recorded + [T.CASES[name](1).plan for name in GOOD]
    wplan_cpp.parser_program(tmp_path, "test_witness_plan_pool", plans, T.bad_plans())
