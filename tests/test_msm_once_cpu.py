"""The table-free MSM's surface, without a device: the three C-ABI calls are declared in include/ezkl_hip.h with the documented signatures,
listed in lib.SYMBOLS and exported by the built library; the Python wrappers exist; and what can be refused without a device is."""
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {
    "ezkl_hip_msm_g1_once_dev": r"int\s+ezkl_hip_msm_g1_once_dev\(ezkl_bases_t h, size_t base_offset, const void\* scalars_dev, size_t n, void\* out_affine, void\* stream\);",
    "ezkl_hip_msm_g1_points_dev": r"int\s+ezkl_hip_msm_g1_points_dev\(const void\* points_dev, const void\* scalars_dev, size_t n, void\* out_affine, void\* stream\);",
    "ezkl_hip_bases_has_table": r"int\s+ezkl_hip_bases_has_table\(ezkl_bases_t h\);",
}


def test_the_calls_are_declared_listed_and_exported():
    from ezkl_amd import lib as L
    header = open(os.path.join(ROOT, "include", "ezkl_hip.h")).read()
    for name, decl in CALLS.items():
        assert L.SYMBOLS.count(name) == 1
        assert re.search(decl, header), "include/ezkl_hip.h does not declare %s with the documented signature" % name
        assert hasattr(L.load(), name)
    assert 'ezkl_hip_last_kernel_ms("msm_once")' in header


def test_the_python_wrappers():
    from ezkl_amd import backend as B
    assert list(inspect.signature(B.Bases.msm_once).parameters)[:4] == ["self", "scalars", "first", "n"]
    assert inspect.signature(B.Bases.msm_once).parameters["first"].default == 0
    assert inspect.signature(B.Bases.msm_once).parameters["n"].default is None
    assert list(inspect.signature(B.msm_points).parameters)[:3] == ["points_dev", "scalars_dev", "n"]
    assert callable(B.Bases.has_table) and callable(B.Bases.msm)
    assert isinstance(B.MSM_ONCE_MIN_POINTS, int) and B.MSM_ONCE_MIN_POINTS >= 0


def test_a_range_outside_the_set_is_refused_before_any_library_call():
    from ezkl_amd import backend as B
    b = B.Bases.__new__(B.Bases)
    b.n, b.h = 10, None                                     # no handle: a call that reached the library would not get far
    for first, n in ((0, 11), (1, 10), (10, 1), (11, None), (-1, 2), (0, -1)):
        with pytest.raises(ValueError, match="of a set of 10 points"):
            b.msm_once(0x1000, first, n)
        with pytest.raises(ValueError, match="of a set of 10 points"):
            b.msm(0x1000, first, n)


def test_null_arguments_are_invalid_without_a_device():
    """the argument checks come before the context: no device is needed to be told EZKL_ERR_INVALID"""
    import ctypes as C
    import numpy as np
    from ezkl_amd import lib as L
    out = np.zeros(8, np.uint64)
    o = out.ctypes.data_as(C.c_void_p)
    lib = L.load()
    assert lib.ezkl_hip_msm_g1_once_dev(None, C.c_size_t(0), C.c_void_p(0x1000), C.c_size_t(1), o, None) == -3
    assert lib.ezkl_hip_msm_g1_points_dev(None, C.c_void_p(0x1000), C.c_size_t(1), o, None) == -3
    assert lib.ezkl_hip_msm_g1_points_dev(C.c_void_p(0x1000), None, C.c_size_t(1), o, None) == -3
    assert lib.ezkl_hip_msm_g1_points_dev(C.c_void_p(0x1000), C.c_void_p(0x1000), C.c_size_t(0), o, None) == -3
    assert lib.ezkl_hip_msm_g1_points_dev(C.c_void_p(0x1008), C.c_void_p(0x1000), C.c_size_t(1), o, None) == -3      # points not 16-byte aligned
    assert lib.ezkl_hip_msm_g1_points_dev(C.c_void_p(0x1000), C.c_void_p(0x1000), C.c_size_t(1), None, None) == -3
    assert lib.ezkl_hip_bases_has_table(None) == 0
