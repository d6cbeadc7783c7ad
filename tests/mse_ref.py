"""numpy model of Mse::Eval (src/aslp-nnet/nnet-loss.cc:205-258) as aslp_mse_eval states it: e, diff and q in float32 with one rounding per
operation (numpy rounds every float32 operation on its own), row sums and totals in float64.  tests/test_mse_ref_cpu.py pins it to the
oracle's orc_mse_eval; the GPU tests compare the kernel, the C ABI and the Python class with it."""
import math

import numpy as np

ROWS = (1, 63, 64, 65, 1000)
COLS = (1, 3, 4, 5, 257, 1024)
SHAPES = [(r, c) for r in ROWS for c in COLS]
WEIGHTS = np.array([0.0, 0.5, 1.0, 2.0], np.float32)
U = 2.0 ** -53   # unit roundoff of the float64 sums


def inputs(rows, cols, seed):
    """net_out, targets [rows x cols] and frame weights drawn from {0, 0.5, 1, 2} with at least one 0 row"""
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((rows, cols)).astype(np.float32)
    t = rng.standard_normal((rows, cols)).astype(np.float32)
    w = rng.choice(WEIGHTS, rows).astype(np.float32)
    w[int(rng.integers(0, rows))] = 0.0
    return y, t, w


def model(y, t, w, scale=1.0):
    """(diff float32, row_loss float64 [rows], total float64): the loss of the minibatch is 0.5 * total"""
    y, t, w = np.asarray(y, np.float32), np.asarray(t, np.float32), np.asarray(w, np.float32)
    wc = w[:, None]
    e = (y - t) * wc
    assert e.dtype == np.float32
    diff = e if scale == 1.0 else e * np.float32(scale)
    q = ((e * e) * wc).astype(np.float64)
    # the correctly rounded sums (math.fsum): a float64 sum of n non-negative terms taken in ANY order lies within (n - 1) 2^-53 relative
    # of the exact sum, hence within n 2^-53 of these -- a model that summed in an order of its own would use up part of that bound
    row_loss = np.array([math.fsum(r) for r in q], np.float64)
    return diff, row_loss, math.fsum(q.ravel())


def num_frames(w):
    """int32 num_frames = frame_weights.Sum(): the weights summed in index order in double, truncated toward zero"""
    s = 0.0
    for x in np.asarray(w, np.float32):
        s += float(x)
    return float(int(s))


def row_bound(cols):
    """relative distance of a float64 sum of `cols` non-negative terms, in any order, from the correctly rounded sum: each of the cols - 1
    additions rounds once, the model's one rounding is the last unit"""
    return cols * U


def total_bound(rows, cols):
    return rows * cols * U

