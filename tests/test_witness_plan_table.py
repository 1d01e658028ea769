"""The table of record kinds is stated once per language: KINDS of ezkl_amd/csrc/witness_plan.hpp, printed by the plain program
tests/cpp/witness_plan_table.cpp, against KINDS of ezkl_amd/witness_plan.py, kind by kind -- name, failure words, unit, span shape -- and the
constants both sides hold.  No device, no library loaded into the interpreter."""
import wplan_cpp


def test_the_two_kind_tables_and_the_shared_constants_are_equal(tmp_path):
    from ezkl_amd import witness_plan as WP
    got = wplan_cpp.run([wplan_cpp.build(tmp_path, "witness_plan_table", ["-O1"])]).stdout.splitlines()
    assert len(WP.KINDS) == WP.KINDS_TOP == 32
    want = ["%d|%s|%s|%s|%d|%d|%s|%s|%d|%d" % (kind, WP.kind_name(kind), K.failure or "-", K.unit, K.scan, K.sparse, K.a, K.b, kind not in WP.UNASSIGNED_KINDS, WP.dst_words(kind, 3, 5))
            for kind, K in enumerate(WP.KINDS)]
    want += ["%s=%d" % (name, getattr(WP, name)) for name in ("SORT_TILE", "MAX_SORT_COUNT", "ARGEXT_CHUNK", "SCATTER_TILE", "MAX_PHASES", "MAX_CHALLENGES", "MAGIC", "VERSION", "KINDS_TOP",
                                                              "NONE")]
    assert got == want
    assert [K.name for K in WP.KINDS] == WP.KIND_NAMES and all((K.name == "?") == (kind in WP.UNASSIGNED_KINDS) for kind, K in enumerate(WP.KINDS))
