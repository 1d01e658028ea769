"""The fixed-base comb without a device: the entry point's name, place in the header, wrapper and refusals, and the two constants the
Python side mirrors from csrc/msm_plan.hpp."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ezkl_hip_g1_fixed_base_dev"


def test_the_entry_point_is_declared_after_downsize_listed_once_exported_and_wrapped():
    from ezkl_amd import backend as B, lib as L
    header = open(os.path.join(ROOT, "include", "ezkl_hip.h")).read()
    decl = re.search(r"int\s+%s\(const void\* base_point, const void\* scalars_dev, size_t n, void\* out_pts_dev, void\* stream\);" % NAME, header)
    assert decl and decl.start() > header.index("int ezkl_hip_bases_downsize(")
    assert 'ezkl_hip_last_kernel_ms("fixed_base")' in header
    assert L.SYMBOLS.count(NAME) == 1
    assert hasattr(L.load(), NAME)
    assert list(inspect.signature(B.g1_fixed_base).parameters) == ["base_point", "scalars_ptr", "n", "out_ptr", "stream"]


def test_the_constants_are_the_header_s():
    from ezkl_amd import backend as B
    plan = open(os.path.join(ROOT, "ezkl_amd", "csrc", "msm_plan.hpp")).read()
    assert int(re.search(r"size_t G1_FIXED_CROSSOVER = (\d+);", plan).group(1)) == B.G1_FIXED_CROSSOVER
    assert int(re.search(r"uint32_t G1_FIXED_C = (\d+);", plan).group(1)) == B.G1_FIXED_C


def test_refusals_need_no_device_and_no_device_is_reported_not_computed():
    from ezkl_amd import lib as L
    f = getattr(L.load(), NAME)
    b, p = (C.c_uint64 * 8)(), C.c_void_p(0x1000)
    for args in ((None, p, 1, p), (b, None, 1, p), (b, p, 0, p), (b, p, 1, None), (b, p, 1, C.c_void_p(0x1008))):
        assert f(args[0], args[1], C.c_size_t(args[2]), args[3], None) == -3                     # EZKL_ERR_INVALID
    if L.load().ezkl_hip_device_count() == 0:                                                     # with a device the call would compute
        assert f(b, p, C.c_size_t(1), p, None) == -1                                              # EZKL_ERR_NO_DEVICE
