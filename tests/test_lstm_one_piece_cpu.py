"""The switch of the one-piece mode of the persistent LSTM recurrences (aslp_lstm_operand_pieces, kaldi-aslp_amd/ops.py lstm_operand_pieces)
without a device: the setter, the getter and the report of the last launch touch no GPU state."""
import ctypes

import pytest


def test_library_exports_and_bindings(aslp):
    for name in ("aslp_lstm_operand_pieces", "aslp_lstm_operand_pieces_get", "aslp_lstm_seq_last_pieces"):
        fn = getattr(aslp.lib, name)          # AttributeError: the library does not export it
        assert fn.argtypes is not None, name  # declared in _lib.py (ctypes leaves argtypes None on an undeclared function)
    assert list(aslp.lib.aslp_lstm_operand_pieces.argtypes) == [ctypes.c_int] and aslp.lib.aslp_lstm_operand_pieces.restype is None
    assert list(aslp.lib.aslp_lstm_operand_pieces_get.argtypes) == [] and aslp.lib.aslp_lstm_operand_pieces_get.restype is ctypes.c_int
    assert list(aslp.lib.aslp_lstm_seq_last_pieces.argtypes) == [] and aslp.lib.aslp_lstm_seq_last_pieces.restype is ctypes.c_int
    assert aslp.lib.aslp_lstm_seq_last_pieces() in (0, 1, 2)   # nothing launched by this thread yet: 0; after other tests of the session 1 or 2


def test_setter_getter_and_context_manager(aslp):
    lib, ops = aslp.lib, aslp.ops
    start = lib.aslp_lstm_operand_pieces_get()
    assert start in (1, 2)
    planes = lib.aslp_gemm_operand_planes_get()
    try:
        ops.set_lstm_operand_pieces(1)
        assert lib.aslp_lstm_operand_pieces_get() == 1
        assert lib.aslp_gemm_operand_planes_get() == planes       # independent of the layer products' switch ...
        ops.set_lstm_operand_pieces(2)
        assert lib.aslp_lstm_operand_pieces_get() == 2
        with ops.operand_planes(1):
            assert lib.aslp_lstm_operand_pieces_get() == 2         # ... in both directions
        with ops.lstm_operand_pieces(1):
            assert lib.aslp_lstm_operand_pieces_get() == 1
            with ops.lstm_operand_pieces(2):
                assert lib.aslp_lstm_operand_pieces_get() == 2
            assert lib.aslp_lstm_operand_pieces_get() == 1
        assert lib.aslp_lstm_operand_pieces_get() == 2
        with pytest.raises(RuntimeError):
            with ops.lstm_operand_pieces(1):
                raise RuntimeError("body failed")
        assert lib.aslp_lstm_operand_pieces_get() == 2            # restored although the body raised
        for other in (7, 0, 3, -5):                                # anything but 1 / 2: back to the environment's choice
            ops.set_lstm_operand_pieces(1 if start == 2 else 2)
            ops.set_lstm_operand_pieces(other)
            assert lib.aslp_lstm_operand_pieces_get() == start, other
    finally:
        ops.set_lstm_operand_pieces(-1)
    assert lib.aslp_lstm_operand_pieces_get() == start
