"""GruStreams (nnet/nnet-recurrent.cpp) under aslp_gru_seq_pieces: the component reaches the persistent kernels through aslp_gru_seq_forward /
_backward, so it follows the switch without a change of its own.  One component (H = 132, 40 inputs, S = 9, T = 5) through two training
steps with momentum and clipping against the oracle chain (oracle_lib.Gru): outputs, input diff and every parameter tensor.
  pieces 2 (and 0):  the bounds of the existing GRU component tests, 1e-4 (the project's fp32 parity bar)
  pieces 1:          derived as tests/test_lstm_one_piece_gpu.py derives them for the LSTM layer: two 11-bit factors allow 2^-10 per product and the
                     recurrence compounds it over the frames, hence 2e-3 against the two-piece run of the same process, tensor by tensor; against
                     the oracle that plus the 1e-4 of the two-piece run.  Not the two-piece bits.
Measured on an MI355X, one piece against two pieces, worst tensor (the second step's outputs): 5.35e-5 relative l2 (MEASURED below)."""
import numpy as np
import pytest
import torch

import nnet_io
from test_rnn_gpu import PERSISTENT, TOL

pytestmark = pytest.mark.gpu
f8 = np.float64
ONE_PIECE = 2e-3
MEASURED = {"one piece against two pieces, worst tensor": 5.35e-5}   # relative l2; printed by the test


def rel(a, b):
    a, b = np.asarray(a, f8), np.asarray(b, f8)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def run(aslp, oracle, dev, tmp_path, pieces):
    """two training steps of the component and of the oracle chain; -> (engine arrays, oracle arrays) as {name: array}"""
    D, H, T, S = 40, 132, 5, 9
    clip, lr, mmt = 0.5, 0.01, 0.9
    rng = np.random.default_rng(17)
    p = oracle.Gru(D, H, rng, scale=0.08)
    g = oracle.Gru(D, H, zero=True)
    path = tmp_path / ("gru%d.nnet" % pieces)
    nnet_io.write_simple_nnet(path, [("<GruStreams>", D, H, nnet_io.gru(p, clip))])
    got, want = {}, {}
    with aslp.ops.gru_seq_pieces(pieces):
        net = aslp.Nnet.Read(path)
        net.SetTrainOptions(learn_rate=lr, momentum=mmt)
        state = np.zeros((S, 5 * H), np.float32)
        for step in range(2):
            x = rng.standard_normal((T * S, D)).astype(np.float32)
            od = rng.standard_normal((T * S, H)).astype(np.float32)
            net.ResetLstmStreams([1] * S if step == 0 else [0] * S)   # the second step starts from the carried h
            buf = p.forward(x, T, S, init_state=state)
            want["out%d" % step] = p.out_of(buf, T, S)
            state = buf[T * S:(T + 1) * S].copy()
            dbuf, want["in_diff%d" % step] = p.backward(od, T, S, buf)
            p.grads(g, x, T, S, buf, dbuf, mmt, clip)
            p.update(g, lr)
            got["out%d" % step] = net.Propagate(torch.from_numpy(x).to(dev)).cpu().numpy()
            assert aslp.lib.aslp_recurrent_last_path(0) == PERSISTENT and aslp.lib.aslp_gru_seq_last_pieces() == pieces, ("forward", step)
            got["in_diff%d" % step] = net.Backpropagate(torch.from_numpy(od).to(dev), want_in_diff=True).cpu().numpy()
            assert aslp.lib.aslp_recurrent_last_path(1) == PERSISTENT and aslp.lib.aslp_gru_seq_last_pieces() == pieces, ("backward", step)
        params = net.GetParams()
    sizes = [t.size for t in p.tensors()]
    for name, part, t in zip(p.NAMES, np.split(params, np.cumsum(sizes)[:-1]), p.tensors()):
        got[name], want[name] = part, t.ravel().copy()
    return got, want


def test_component_follows_the_switch(aslp, oracle, dev, tmp_path):
    runs = {}
    try:
        for pieces in (2, 0, 1):
            runs[pieces] = run(aslp, oracle, dev, tmp_path, pieces)
    finally:
        aslp.ops.set_gru_seq_pieces(-1)
    assert aslp.lib.aslp_gru_seq_pieces_get() == 0
    names = sorted(runs[2][0])
    assert {"out0", "out1", "in_diff0", "in_diff1", "w_zrm_x", "w_zr_h", "w_m_g", "bias"} == set(names)
    for pieces in (2, 0):
        got, want = runs[pieces]
        for name in names:
            assert np.isfinite(got[name]).all() and oracle.rel_err(got[name], want[name]) < TOL, (pieces, name, oracle.rel_err(got[name], want[name]))
    one, want = runs[1]
    two = runs[2][0]
    worst = 0.0
    for name in names:
        r2, ro = rel(one[name], two[name]), oracle.rel_err(one[name], want[name])
        worst = max(worst, r2)
        print("GruStreams one piece, %s: against two pieces %.3e, against the oracle %.3e" % (name, r2, ro))
        assert np.isfinite(one[name]).all() and r2 < ONE_PIECE and ro < ONE_PIECE + TOL, (name, r2, ro)
    print("GruStreams one piece against two pieces, worst tensor: %.3e" % worst)
    assert not all(np.array_equal(one[n], two[n]) for n in names)
    assert not np.array_equal(one["out0"], two["out0"])     # h(0) = 0 at the first step, but g(t) m-product and the steps behind it are rounded
