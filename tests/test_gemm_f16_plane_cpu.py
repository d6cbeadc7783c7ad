"""The one-plane product mode's switch (aslp_gemm_operand_planes, kaldi-aslp_amd/ops.py operand_planes) without a device: the setter and the
getter touch no GPU state."""
import ctypes

import pytest


def test_library_exports_and_bindings(aslp):
    for name in ("aslp_gemm_operand_planes", "aslp_gemm_operand_planes_get"):
        fn = getattr(aslp.lib, name)          # AttributeError: the library does not export it
        assert fn.argtypes is not None, name  # declared in _lib.py (ctypes leaves argtypes None on an undeclared function)
    assert list(aslp.lib.aslp_gemm_operand_planes.argtypes) == [ctypes.c_int] and aslp.lib.aslp_gemm_operand_planes.restype is None
    assert list(aslp.lib.aslp_gemm_operand_planes_get.argtypes) == [] and aslp.lib.aslp_gemm_operand_planes_get.restype is ctypes.c_int


def test_setter_getter_and_context_manager(aslp, monkeypatch):
    lib, ops = aslp.lib, aslp.ops
    start = lib.aslp_gemm_operand_planes_get()
    assert start in (1, 2)
    try:
        ops.set_operand_planes(1)
        assert lib.aslp_gemm_operand_planes_get() == 1
        ops.set_operand_planes(2)
        assert lib.aslp_gemm_operand_planes_get() == 2
        with ops.operand_planes(1):
            assert lib.aslp_gemm_operand_planes_get() == 1
            with ops.operand_planes(2):
                assert lib.aslp_gemm_operand_planes_get() == 2
            assert lib.aslp_gemm_operand_planes_get() == 1
        assert lib.aslp_gemm_operand_planes_get() == 2
        with pytest.raises(RuntimeError):
            with ops.operand_planes(1):
                raise RuntimeError("body failed")
        assert lib.aslp_gemm_operand_planes_get() == 2      # restored although the body raised
        ops.set_operand_planes(7)                            # anything but 1 / 2: back to the environment's choice
        assert lib.aslp_gemm_operand_planes_get() == start
    finally:
        ops.set_operand_planes(-1)
    assert lib.aslp_gemm_operand_planes_get() == start
