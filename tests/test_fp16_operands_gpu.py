"""One training step under the one switch for fp16 operands (ops.fp16_operands(1) / aslp_fp16_operands): a net that holds every product site
the switch reaches -- a layer product the split path serves (256 x 128 -> 128), an LstmProjectedStreams at 1028 cells (per-timestep path)
and a GruStreams at 1028 units (per-timestep path).  Inside the block the layer products run on a one-plane tile, the LSTM step kernels
multiply with one piece and so do the GRU step kernels (aslp_gru_step_pieces joins the umbrella: its one-piece form measured faster,
DESIGN section 7), and the step stays within lstm_seq_ref.BAR_ONE_PIECE (relative l2 2e-3, element 2e-2) of the same step outside the block."""
import numpy as np
import pytest
import torch

import nnet_io
from lstm_seq_ref import BAR_ONE_PIECE
from test_rnn_paths_gpu import STEP_FUSED

pytestmark = pytest.mark.gpu

ONE_PLANE_TILES, TWO_PLANE_TILES = (404, 408, 411), (304, 308, 311, 328, 351)
D, A, CELLS, R, H, T, S = 128, 128, 1028, 64, 1028, 8, 32
GRU_STEP_PIECES_UNDER_UMBRELLA = 1


def write_net(oracle, path):
    rng = np.random.default_rng(9)
    lstm = oracle.LstmDir(A, CELLS, R, False, rng, scale=0.05)
    gru = oracle.Gru(R, H, rng, scale=0.05)
    W, b = (rng.standard_normal((A, D)) * 0.1).astype(np.float32), (rng.standard_normal(A) * 0.1).astype(np.float32)
    nnet_io.write_simple_nnet(path, [("<AffineTransform>", D, A, nnet_io.affine(W, b)),
                                     ("<LstmProjectedStreams>", A, R, nnet_io.lstm([lstm], 1.0, CELLS)),
                                     ("<GruStreams>", R, H, nnet_io.gru(gru, 1.0))])


def one_step(aslp, dev, path, x, od, tiles, lstm_pieces, gru_pieces):
    net = aslp.Nnet.Read(str(path))
    net.SetTrainOptions(learn_rate=1e-3, momentum=0.9)
    net.ResetLstmStreams([1] * S)
    out = net.Propagate(torch.from_numpy(x).to(dev)).cpu().numpy()
    assert aslp.lib.aslp_recurrent_last_path(0) == STEP_FUSED
    assert (aslp.lib.aslp_lstm_step_last_pieces(), aslp.lib.aslp_gru_step_last_pieces()) == (lstm_pieces, gru_pieces), "forward"
    idf = net.Backpropagate(torch.from_numpy(od).to(dev), want_in_diff=True).cpu().numpy()
    assert aslp.lib.aslp_recurrent_last_path(1) == STEP_FUSED
    assert (aslp.lib.aslp_lstm_step_last_pieces(), aslp.lib.aslp_gru_step_last_pieces()) == (lstm_pieces, gru_pieces), "backward"
    assert aslp.lib.aslp_gemm_last_tile() in tiles, aslp.lib.aslp_gemm_last_tile()   # the step's latest product: the layer's weight gradient
    return out, idf, np.asarray(net.GetParams(), np.float32)


def test_one_training_step_under_the_umbrella(aslp, oracle, dev, tmp_path):
    path = tmp_path / "net.nnet"
    write_net(oracle, path)
    rng = np.random.default_rng(10)
    x = rng.standard_normal((T * S, D)).astype(np.float32)
    od = (rng.standard_normal((T * S, H)) * 0.1).astype(np.float32)
    aslp.ops.set_fp16_operands(-1)
    assert aslp.lib.aslp_fp16_operands_get() == 0, "the suite runs with ASLP_FP16_OPERANDS unset"
    try:
        outside = one_step(aslp, dev, path, x, od, TWO_PLANE_TILES, 0, 0)
        with aslp.ops.fp16_operands(1):
            inside = one_step(aslp, dev, path, x, od, ONE_PLANE_TILES, 1, GRU_STEP_PIECES_UNDER_UMBRELLA)
            with aslp.ops.gru_step_pieces(0):          # the site's own switch still wins inside the block
                both = one_step(aslp, dev, path, x, od, ONE_PLANE_TILES, 1, 0)
            aslp.ops.set_gru_step_pieces(-1)           # (the inner block pinned what was in force on its exit: hand the choice back)
        again = one_step(aslp, dev, path, x, od, TWO_PLANE_TILES, 0, 0)
    finally:
        aslp.ops.set_fp16_operands(-1)
        aslp.ops.set_gru_step_pieces(-1)
    assert all(np.array_equal(a, b) for a, b in zip(outside, again)), "the block left something behind"
    for what, got in (("umbrella", inside), ("umbrella + gru_step_pieces(0)", both)):
        worst = {}
        for name, a, b in zip(("out", "in_diff", "params"), got, outside):
            assert np.isfinite(a).all(), (what, name)
            l2, el = oracle.rel_err(a, b), oracle.max_err(a, b)
            worst[name] = (l2, el)
            assert l2 < BAR_ONE_PIECE and el < 10 * BAR_ONE_PIECE, (what, name, l2, el)
        assert not np.array_equal(got[0], outside[0]), (what, "the switch reached no product")
        print("fp16-operands %s vs outside (relative l2 / element): " % what + "  ".join("%s %.1e / %.1e" % ((k,) + v) for k, v in worst.items()))
    assert not np.array_equal(both[0], inside[0])
