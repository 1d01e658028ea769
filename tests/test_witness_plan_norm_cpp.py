"""The C++ parser's RECIP / ISQRT rules (ezkl_amd/csrc/witness_plan.hpp) as a plain program under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/cpp/test_witness_plan_norm.cpp reads the blobs written here -- synthetic plans of the new kinds it must
take, the plans recorded from a NormCircuit (softmax and layer norm), and every plan of witness_synth_norm.bad_plans() with the message the
Python validator gave for it -- and says what it asserts.  No device, no library loaded into the interpreter, no preload."""
import witness_synth_norm as T
import wplan_cpp

GOOD = ["recip-n1-S1", "recip-n65-S2097152", "recip-n257-S%d" % ((1 << 62) - 1), "sqrt-n1-scale1", "sqrt-n64-scale128", "sqrt-n257-scale%d" % ((1 << 31) - 1)]


def test_the_norm_rules_of_the_parser_under_the_sanitizers(tmp_path):
    from ezkl_amd import ezkl_layout as EL, witness_plan as WP
    recorded = [WP.record_plan(EL.NormCircuit(9, 2, 3000, 2, 4, layer_norm=ln)) for ln in (False, True)]
    plans = [T.small_plan().plan, T.failing_case(WP.RECIP, 1 << 21, True).plan, T.failing_case(WP.ISQRT, 128, True).plan] + recorded + [T.CASES[name](1).plan for name in GOOD]
    wplan_cpp.parser_program(tmp_path, "test_witness_plan_norm", plans, T.bad_plans())
