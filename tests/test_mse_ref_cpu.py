"""tests/mse_ref.py (the numpy model the Mse GPU tests compare with) against the oracle's orc_mse_eval (oracle/aslp_oracle.c, the reference's
CPU arithmetic restated in C), on the shapes the GPU tests use: the same diff bit for bit, the same frame count, and a loss inside the
bound of a float64 sum of rows * cols non-negative terms taken in another order."""
import ctypes as C

import numpy as np
import pytest

import mse_ref


@pytest.mark.parametrize("rows,cols", mse_ref.SHAPES)
def test_model_matches_oracle(oracle, rows, cols):
    y, t, w = mse_ref.inputs(rows, cols, 1000 * rows + cols)
    diff, row_loss, total = mse_ref.model(y, t, w)
    ref_diff = np.empty((rows, cols), np.float32)
    loss, frames = C.c_double(), C.c_double()
    oracle.lib.orc_mse_eval(w, y, cols, t, cols, rows, cols, ref_diff, cols, C.byref(loss), C.byref(frames))
    assert np.array_equal(diff.view(np.uint32), ref_diff.view(np.uint32))
    assert frames.value == mse_ref.num_frames(w)
    assert abs(0.5 * total - loss.value) <= mse_ref.total_bound(rows, cols) * loss.value
    assert row_loss.shape == (rows,) and (row_loss >= 0).all() and (row_loss[w == 0] == 0).all()


def test_scale_is_a_second_rounding(oracle):
    """MultiTaskLoss' Scale: the oracle multiplies the finished diff block by the task weight"""
    y, t, w = mse_ref.inputs(65, 5, 7)
    diff, _, total = mse_ref.model(y, t, w, 0.25)
    plain, _, total1 = mse_ref.model(y, t, w)
    assert np.array_equal(diff, plain * np.float32(0.25)) and total == total1
    spec = [("mse", 5, 0.25)]
    d, st = oracle.multitask_eval(spec, w, y, t)
    assert np.array_equal(np.asarray(d, np.float32).view(np.uint32), diff.view(np.uint32))
    assert abs(0.5 * total - st[0]["loss"]) <= mse_ref.total_bound(65, 5) * st[0]["loss"] and st[0]["frames"] == mse_ref.num_frames(w)


def test_frames_truncate_per_minibatch():
    w = np.array([0.5, 2.0, 0.0], np.float32)
    assert mse_ref.num_frames(w) == 2.0
