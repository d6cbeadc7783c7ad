"""The opt-in one-piece mode of the persistent LSTM recurrences (aslp_lstm_operand_pieces(1), ASLP_LSTM_PIECES=1; csrc/rnn_persistent.hip
lstm_seq_fwd_h / lstm_seq_bwd_h with NP = 1): the recurrent product reads fp16(m(t-1)) and fp16(W sc) / sc (backward: fp16(dG s) / s and the hi
piece of the W_eff rows) and accumulates in fp32; everything outside the product is the same fp32 code.  The default (two pieces) must not
change by a bit, the one-piece results must be what that operand model says, and the hand-off between workgroups must be untouched."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nnet_io
from test_ab_switches_gpu import run as run_lc_child          # two chunks of an LC-BLSTM layer in a child process (switches read once per process)
from test_rnn_gpu import FAMILY, PERSISTENT, build

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f8 = np.float64


def rel(a, b):
    a, b = np.asarray(a, f8), np.asarray(b, f8)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def fp16(v):
    """round to nearest even like v_cvt_f16_f32; the values here are fp32 numbers or fp32 numbers times a power of two"""
    return np.asarray(v, np.float32).astype(np.float16).astype(f8)


def pow2_scale(amax):
    """the power of two that puts amax in [2^13, 2^14) (rnn_persistent.hip: frexpf, ldexpf(1, 14 - e)); 1 where there is nothing to scale"""
    amax = np.asarray(amax, f8)
    _, e = np.frexp(amax)
    return np.where(amax > 0, np.ldexp(1.0, 14 - e), 1.0)


def round_weight_rows(w):
    """fp16(w sc) / sc with sc per gate column = per row of the [G C, K] recurrent matrix"""
    sc = pow2_scale(np.abs(w).max(axis=1))[:, None]
    return fp16(np.asarray(w, np.float32) * sc.astype(np.float32)) / sc


def train_chunks(aslp, dev, path, marker, D, out_dim, T, S, nchunks=2, chunk=0, seed=7, lens=None, lr=1e-3, od_scale=0.1):
    """nchunks x (Propagate, Backpropagate + update) of one layer read from `path`; returns the arrays and the piece counts that ran"""
    bidir, proj, cifg, lc, _ = FAMILY.get(marker, (False, False, False, False, False))
    net = aslp.Nnet.Read(path)
    net.SetTrainOptions(learn_rate=lr, momentum=0.9)
    if lc:
        net.SetChunkSize(chunk)
    rng = np.random.default_rng(seed)
    arrays, pieces, paths = [], [], []
    for step in range(nchunks):
        x = rng.standard_normal((T * S, D)).astype(np.float32)
        od = (rng.standard_normal((T * S, out_dim)) * od_scale).astype(np.float32)
        if bidir and not lc:
            net.SetSeqLengths(lens)
        else:
            net.ResetLstmStreams([1] * S if step == 0 else [0] * S)
        arrays.append(net.Propagate(torch.from_numpy(x).to(dev)).cpu().numpy())
        pieces.append(aslp.lib.aslp_lstm_seq_last_pieces()); paths.append(aslp.lib.aslp_recurrent_last_path(0))
        arrays.append(net.Backpropagate(torch.from_numpy(od).to(dev), want_in_diff=True).cpu().numpy())
        pieces.append(aslp.lib.aslp_lstm_seq_last_pieces()); paths.append(aslp.lib.aslp_recurrent_last_path(1))
    arrays.append(net.GetParams())
    return arrays, pieces, paths


def clean_error(aslp):
    import ctypes
    buf = ctypes.create_string_buffer(1024)
    rc = aslp.lib.aslp_get_last_error(buf, 1024)
    return rc == 0, buf.value.decode()


def test_default_untouched(aslp, oracle, dev, tmp_path):
    """1. nothing set, pieces(2), and pieces(1) taken back again: the same bits, and two pieces are what ran"""
    marker, D, Cc, R, T, S, chunk = "<BLstmProjectedStreamsLC>", 40, 128, 64, 9, 16, 6
    _, _, out_dim, path = build(oracle, tmp_path, marker, D, Cc, R, 5.0, seed=4, scale=0.05)
    aslp.ops.set_lstm_operand_pieces(-1)
    assert aslp.lib.aslp_lstm_operand_pieces_get() == 2, "the suite runs with ASLP_LSTM_PIECES unset"
    try:
        base, pieces, paths = train_chunks(aslp, dev, path, marker, D, out_dim, T, S, chunk=chunk)
        assert set(paths) == {PERSISTENT} and set(pieces) == {2}, (paths, pieces)
        with aslp.ops.lstm_operand_pieces(2):
            two, pieces, _ = train_chunks(aslp, dev, path, marker, D, out_dim, T, S, chunk=chunk)
        assert set(pieces) == {2}
        aslp.ops.set_lstm_operand_pieces(1); aslp.ops.set_lstm_operand_pieces(-1)
        back, pieces, _ = train_chunks(aslp, dev, path, marker, D, out_dim, T, S, chunk=chunk)
        assert set(pieces) == {2}
        with aslp.ops.lstm_operand_pieces(1):
            one, pieces, _ = train_chunks(aslp, dev, path, marker, D, out_dim, T, S, chunk=chunk)
        assert set(pieces) == {1}
    finally:
        aslp.ops.set_lstm_operand_pieces(-1)
    for a, b, c in zip(base, two, back):
        assert np.isfinite(a).all() and np.array_equal(a, b) and np.array_equal(a, c)
    assert not all(np.array_equal(a, b) for a, b in zip(base, one))    # ... and the switch does reach the kernels


def test_forward_operand_model(aslp, oracle, dev, tmp_path):
    """2. One recurrent product with known operands: a non-projected <Lstm> (its output is the m the recurrence multiplies) at C = 512, S = 32,
    two Propagate calls of T = 1 -- the first after a reset (no recurrent term), the second from the carried state.  The second step in float64,
    (a) with the operands as they are and (b) with fp16(m(1)) and fp16(W sc) / sc, m(1) being the first call's output as read back (so the
    operand is exact) and c(1) the float64 model's.  e2 = the two-piece kernel's error against (a), measured here.  One piece: against (b)
    <= 4 e2 + 2e-7 (the same arithmetic, other operands), against (a) >= 20 x its error against (b) (the mode really rounds)."""
    marker, D, Cc, S = "<Lstm>", 40, 512, 32
    dirs, _, out_dim, path = build(oracle, tmp_path, marker, D, Cc, 0, 5.0, seed=21, scale=0.05)
    d = dirs[0]
    rng = np.random.default_rng(8)
    x1, x2 = (rng.standard_normal((S, D)).astype(np.float32) for _ in range(2))
    wx, wr, b = d.w_x.astype(f8), d.w_r.astype(f8), d.bias.astype(f8)
    pi, pf, po = d.peep_i.astype(f8), d.peep_f.astype(f8), d.peep_o.astype(f8)

    def cell(pre, c):
        g, i, f = np.tanh(pre[:, :Cc]), sig(pre[:, Cc:2 * Cc] + c * pi), sig(pre[:, 2 * Cc:3 * Cc] + c * pf)
        c = np.clip(g * i + c * f, -50.0, 50.0)
        return sig(pre[:, 3 * Cc:] + c * po) * np.tanh(c), c

    m1_model, c1 = cell(x1.astype(f8) @ wx.T + b, np.zeros((S, Cc)))
    got = {}
    try:
        for n in (2, 1):
            with aslp.ops.lstm_operand_pieces(n):
                net = aslp.Nnet.Read(path)
                net.ResetLstmStreams([1] * S)
                m1 = net.Propagate(torch.from_numpy(x1).to(dev)).cpu().numpy()
                net.ResetLstmStreams([0] * S)
                m2 = net.Propagate(torch.from_numpy(x2).to(dev)).cpu().numpy()
                assert aslp.lib.aslp_recurrent_last_path(0) == PERSISTENT and aslp.lib.aslp_lstm_seq_last_pieces() == n
                got[n] = (m1, m2)
    finally:
        aslp.ops.set_lstm_operand_pieces(-1)
    assert rel(got[2][0], m1_model) < 5e-6 and np.array_equal(got[1][0], got[2][0])    # the first step holds no recurrent product
    xpart = x2.astype(f8) @ wx.T + b
    err = {}
    for n in (2, 1):
        m1 = got[n][0].astype(f8)
        model_a, _ = cell(xpart + m1 @ wr.T, c1)
        model_b, _ = cell(xpart + fp16(m1) @ round_weight_rows(d.w_r).T, c1)
        err[n] = (rel(got[n][1], model_a), rel(got[n][1], model_b))
    e2 = err[2][0]
    print("forward operand model: two pieces vs (a) %.3e (vs (b) %.3e); one piece vs (a) %.3e, vs (b) %.3e" % (e2, err[2][1], err[1][0], err[1][1]))
    assert e2 < 5e-6, err
    assert err[1][1] <= 4 * e2 + 2e-7, err
    assert err[1][0] >= 20 * err[1][1], err


def test_long_sequence_difference_and_reproducibility(aslp, oracle, dev, tmp_path):
    """3. cfg3 widths (LstmProjectedStreams C = 512, R = 256, T = 60, S = 32, the inputs of test_recurrent_products_against_float64): rounding
    flips of the fp16 operands amplify over 60 steps, so a comparison with the rounded model cannot be sharp -- only: finite, the difference
    from the two-piece run inside (1e-5, 1e-3), and two one-piece runs bit-identical."""
    D, Cc, R, T, S = 40, 512, 256, 60, 32
    marker = "<LstmProjectedStreams>"
    _, _, out_dim, path = build(oracle, tmp_path, marker, D, Cc, R, 5.0, seed=21, scale=0.05)
    x = torch.from_numpy(np.random.default_rng(8).standard_normal((T * S, D)).astype(np.float32)).to(dev)
    outs = []
    try:
        for n in (2, 1, 1):
            with aslp.ops.lstm_operand_pieces(n):
                net = aslp.Nnet.Read(path)
                net.ResetLstmStreams([1] * S)
                outs.append(net.Propagate(x).cpu().numpy())
                assert aslp.lib.aslp_recurrent_last_path(0) == PERSISTENT and aslp.lib.aslp_lstm_seq_last_pieces() == n
    finally:
        aslp.ops.set_lstm_operand_pieces(-1)
    diff = rel(outs[1], outs[0])
    print("T = 60: one piece against two pieces %.3e (last frame %.3e)" % (diff, rel(outs[1][-S:], outs[0][-S:])))
    assert all(np.isfinite(o).all() for o in outs)
    assert 1e-5 < diff < 1e-3, diff
    assert np.array_equal(outs[1], outs[2])


def test_backward_operand_model(aslp, oracle, dev, tmp_path):
    """4. One backward product: <Lstm> (one direction, W_eff = W_r, read back from the net) at C = 128, S = 8, T = 2, no clipping.  The float64
    model of forward and backward, (a) with the operands as they are and (b) with the one-piece operands -- forward fp16(m(1)) (the GPU's own
    m(1)) and fp16(W sc) / sc per gate column, backward fp16(dG(2) s) / s per stream and the hi piece of the W_eff rows behind the per-column
    scale of the workgroup's 16-cell x G row block.  The one-piece in-diff must be at least 5 x closer to (b) than to (a); the two-piece in-diff
    stays at its fp32 level against (a).  Both pairs of errors are printed before the assertions (whole in-diff, and the rows of t = 1 that the
    product reaches)."""
    marker, D, Cc, S, T = "<Lstm>", 24, 128, 8, 2
    dirs, _, out_dim, path = build(oracle, tmp_path, marker, D, Cc, 0, 0.0, seed=5, scale=0.1)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((T * S, D)).astype(np.float32)
    od = (rng.standard_normal((T * S, Cc)) * 0.1).astype(np.float32)
    got = {}
    try:
        for n in (2, 1):
            with aslp.ops.lstm_operand_pieces(n):
                net = aslp.Nnet.Read(path)
                net.SetTrainOptions(learn_rate=0.0, momentum=0.0)
                params = net.GetParams()
                net.ResetLstmStreams([1] * S)
                out = net.Propagate(torch.from_numpy(x).to(dev)).cpu().numpy()
                idf = net.Backpropagate(torch.from_numpy(od).to(dev), want_in_diff=True).cpu().numpy()
                assert aslp.lib.aslp_recurrent_last_path(1) == PERSISTENT and aslp.lib.aslp_lstm_seq_last_pieces() == n
                got[n] = (out, idf)
    finally:
        aslp.ops.set_lstm_operand_pieces(-1)
    # the GPU's own parameters, file order: W_x, W_r, bias, peepholes i / f / o
    G = 4
    sizes = [G * Cc * D, G * Cc * Cc, G * Cc, Cc, Cc, Cc]
    parts = np.split(params.astype(np.float32), np.cumsum(sizes)[:-1])
    wx32, wr32 = parts[0].reshape(G * Cc, D), parts[1].reshape(G * Cc, Cc)
    wx, wr, b, pi, pf, po = wx32.astype(f8), wr32.astype(f8), parts[2].astype(f8), parts[3].astype(f8), parts[4].astype(f8), parts[5].astype(f8)
    # backward B operand: W_eff[gate * C + cell, col], scaled per output column col within a workgroup's row block (16 cells x G gates)
    wr_b = np.empty_like(wr)
    for c0 in range(0, Cc, 16):
        rows = np.concatenate([np.arange(g * Cc + c0, g * Cc + c0 + 16) for g in range(G)])
        blk = wr32[rows]
        sc = pow2_scale(np.abs(blk).max(axis=0))[None, :]
        wr_b[rows] = fp16(blk * sc.astype(np.float32)) / sc
    dsigm = lambda y, dd: dd * y * (1.0 - y)
    dtanh = lambda y, dd: dd * (1.0 - y * y)

    def model(rounded, m1_gpu):
        xs = [x[t * S:(t + 1) * S].astype(f8) for t in range(T)]
        ods = [od[t * S:(t + 1) * S].astype(f8) for t in range(T)]
        st, c, m = [], np.zeros((S, Cc)), None
        for t in range(T):
            pre = xs[t] @ wx.T + b
            if t == 1:
                pre = pre + ((fp16(m1_gpu) @ round_weight_rows(wr32).T) if rounded else (m @ wr.T))
            g, i, f = np.tanh(pre[:, :Cc]), sig(pre[:, Cc:2 * Cc] + c * pi), sig(pre[:, 2 * Cc:3 * Cc] + c * pf)
            cn = g * i + c * f
            o = sig(pre[:, 3 * Cc:] + cn * po)
            h = np.tanh(cn)
            st.append(dict(g=g, i=i, f=f, o=o, h=h, c=cn, cprev=c))
            c, m = cn, o * h
        idf, dG_next, nxt = [None] * T, None, None
        for t in (1, 0):
            y = st[t]
            dm = ods[t].copy()
            if dG_next is not None:
                if rounded:   # per stream: the largest of the workgroup's 16 * G values of that stream goes to [2^13, 2^14)
                    share = np.zeros((S, Cc))
                    for c0 in range(0, Cc, 16):
                        cols = np.concatenate([np.arange(g * Cc + c0, g * Cc + c0 + 16) for g in range(G)])
                        blk = dG_next[:, cols]
                        s_ = pow2_scale(np.abs(blk).max(axis=1))[:, None]
                        share += (fp16((blk * s_).astype(np.float32)) / s_) @ wr_b[cols]
                    dm += share
                else:
                    dm += dG_next @ wr
            dh = dtanh(y["h"], dm * y["o"])
            do = dsigm(y["o"], dm * y["h"])
            dc = dh + do * po
            if nxt is not None:
                dc = dc + nxt["dc"] * st[t + 1]["f"] + nxt["di"] * pi + nxt["df"] * pf
            df, di, dg = dsigm(y["f"], dc * y["cprev"]), dsigm(y["i"], dc * y["g"]), dtanh(y["g"], dc * y["i"])
            dG = np.concatenate([dg, di, df, do], axis=1)
            idf[t] = dG @ wx
            dG_next, nxt = dG, dict(dc=dc, di=di, df=df)
        return np.concatenate([s_["o"] * s_["h"] for s_ in st], axis=0), np.concatenate(idf, axis=0)

    res = {}
    for n in (2, 1):
        out, idf = got[n]
        (_, idf_a), (_, idf_b) = model(False, None), model(True, out[:S])
        res[n] = (rel(idf, idf_a), rel(idf, idf_b), rel(idf[:S], idf_a[:S]), rel(idf[:S], idf_b[:S]))
        print("backward operand model, %d piece(s): in-diff vs (a) %.3e, vs (b) %.3e; rows of t = 1 alone: vs (a) %.3e, vs (b) %.3e" % ((n,) + res[n]))
    assert res[2][0] < 5e-6, res
    assert res[1][1] <= res[1][0] / 5.0, res


@pytest.mark.parametrize("pscale,odscale,lr", [("0.3", "1e-9", "1e-3"), ("0.001", "1e5", "1e-12"), ("0.05", "1e-20", "1e-3"), ("0.2", "30.0", "1e-6")])
def test_one_piece_at_any_magnitude(tmp_path, pscale, odscale, lr):
    """5. The cases of test_split_f16_products_keep_fp32_accuracy_at_any_magnitude under ASLP_LSTM_PIECES=1: the power-of-two scales (weights per
    column, gate diffs per stream and timestep) are the two-piece kernels', so nothing depends on the operands' size.  Bound 2e-3 blockwise: two
    11-bit factors allow 2^-10 per product, the recurrence compounds it over the 9 frames, hence twice that."""
    env = dict(AB_PSCALE=pscale, AB_ODSCALE=odscale, AB_LR=lr, AB_CLIP="0.0")
    two = run_lc_child(tmp_path, "two", **env)
    one = run_lc_child(tmp_path, "one", ASLP_LSTM_PIECES="1", **env)
    assert np.isfinite(one).all() and np.isfinite(two).all()
    assert not np.array_equal(one, two)
    n = 2 * (9 * 16 * 128 + 9 * 16 * 24)        # outputs and input diffs of the two chunks, then the parameters
    blocks = [(o + lo, o + hi) for o in (0, n // 2) for lo, hi in ((0, 9 * 16 * 128), (9 * 16 * 128, 9 * 16 * (128 + 24)))] + [(n, len(one))]
    for lo, hi in blocks:
        a, b = one[lo:hi].astype(f8), two[lo:hi].astype(f8)
        r = np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)
        print("pscale %s odscale %s lr %s block [%d, %d): one piece against two %.3e" % (pscale, odscale, lr, lo, hi, r))
        assert np.linalg.norm(a - b) <= 2e-3 * np.linalg.norm(b) + 1e-30, (lo, hi, r)


MEMBERS = ["<LstmProjectedStreams>", "<LstmCifgProjectedStreams>", "<Lstm>", "<BLstm>", "<BLstmProjectedStreams>", "<BLstmProjectedStreamsLC>"]


@pytest.mark.parametrize("marker", MEMBERS)
def test_family_runs_one_piece(aslp, oracle, dev, tmp_path, marker):
    """6. every member trains a step with one piece (the bidirectional non-LC ones with ragged lengths), stays finite and reports what ran: 1,
    and 0 where aslp_lstm_split16(0) put the products on the fp32 instruction -- that switch wins"""
    D, Cc, R, T, S = 40, 128, 64, 9, 16
    bidir, proj, cifg, lc, _ = FAMILY[marker]
    _, _, out_dim, path = build(oracle, tmp_path, marker, D, Cc, R if proj else 0, 5.0, seed=6, scale=0.05)
    lens = np.random.default_rng(2).integers(1, T + 1, S).astype(np.int32)
    lens[0] = T
    try:
        with aslp.ops.lstm_operand_pieces(1):
            one, pieces, paths = train_chunks(aslp, dev, path, marker, D, out_dim, T, S, chunk=6, lens=lens)
            assert set(paths) == {PERSISTENT} and set(pieces) == {1}, (marker, paths, pieces)
            aslp.lib.aslp_lstm_split16(0)
            f32, pieces, paths = train_chunks(aslp, dev, path, marker, D, out_dim, T, S, chunk=6, lens=lens)
            assert set(paths) == {PERSISTENT} and set(pieces) == {0}, (marker, paths, pieces)
    finally:
        aslp.lib.aslp_lstm_split16(-1)
        aslp.ops.set_lstm_operand_pieces(-1)
    two, pieces, _ = train_chunks(aslp, dev, path, marker, D, out_dim, T, S, chunk=6, lens=lens)
    assert set(pieces) == {2}
    for a, b, c in zip(one, two, f32):
        assert np.isfinite(a).all()
        assert rel(a, b) < 2e-3, (marker, rel(a, b))
        assert rel(c, b) < 1e-5, (marker, rel(c, b))            # under split16(0) the piece switch changes nothing: the fp32 kernels' values
    assert not all(np.array_equal(a, b) for a, b in zip(one, two))


def test_per_timestep_path_and_gru_keep_their_bits(aslp, oracle, dev, tmp_path):
    """6. (continued) where the persistent LSTM kernels do not run the switch has no effect: the per-timestep path (ASLP_LSTM_PERSISTENT=0, read
    once per process: child processes) and GruStreams give the same bits with and without it"""
    a = run_lc_child(tmp_path, "step_two", ASLP_LSTM_PERSISTENT="0")
    b = run_lc_child(tmp_path, "step_one", ASLP_LSTM_PERSISTENT="0", ASLP_LSTM_PIECES="1")
    assert np.isfinite(a).all() and np.array_equal(a, b)
    D, H, T, S = 24, 128, 12, 16
    rng = np.random.default_rng(9)
    p = oracle.Gru(D, H, rng, scale=0.08)
    path = tmp_path / "gru.nnet"
    nnet_io.write_simple_nnet(path, [("<GruStreams>", D, H, nnet_io.gru(p, 0.5))])
    base, _, _ = train_chunks(aslp, dev, path, "<GruStreams>", D, H, T, S)
    try:
        with aslp.ops.lstm_operand_pieces(1):
            other, _, _ = train_chunks(aslp, dev, path, "<GruStreams>", D, H, T, S)
    finally:
        aslp.ops.set_lstm_operand_pieces(-1)
    for x, y in zip(base, other):
        assert np.isfinite(x).all() and np.array_equal(x, y)


TRAIN_CHILD = r'''
import sys, json, os
import numpy as np, torch
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import aslp_import
aslp = aslp_import.load(); aslp.ops.use_torch_stream()
dev = torch.device("cuda:0")
S, chunk, T, D, A = 16, 6, 8, 64, 64     # T S = 128 rows, every width a multiple of 64: the layer products run on the split-fp16 kernels
proto = """<NnetProto>
<BLstmProjectedStreamsLC> <InputDim> 64 <OutputDim> 128 <CellDim> 128 <ParamScale> 0.05 <ClipGradient> 5.0
<BLstmProjectedStreamsLC> <InputDim> 128 <OutputDim> 128 <CellDim> 128 <ParamScale> 0.05 <ClipGradient> 5.0
<AffineTransform> <InputDim> 128 <OutputDim> 64 <BiasMean> 0.0 <BiasRange> 0.0 <ParamStddev> 0.1
<Softmax> <InputDim> 64 <OutputDim> 64
</NnetProto>
"""
net = aslp.Nnet.Init(proto, seed=5)
net.SetTrainOptions(learn_rate=2e-4, momentum=0.9)
net.SetChunkSize(chunk)
g = torch.Generator(device="cpu"); g.manual_seed(3)
proj = torch.randn(D, A, generator=g)
losses, pieces = [], set()
for step in range(50):
    x = torch.randn(T * S, D, generator=g)
    lab = (x @ proj).argmax(dim=1)                     # learnable targets: the loss falls over the 50 steps
    net.ResetLstmStreams([1] * S if step %% 5 == 0 else [0] * S)
    p = net.Propagate(x.to(dev)).cpu()
    pieces.add(int(aslp.lib.aslp_lstm_seq_last_pieces()))
    losses.append(float(-torch.log(p[torch.arange(T * S), lab].double().clamp_min(1e-30)).mean()))
    diff = p.clone(); diff[torch.arange(T * S), lab] -= 1.0   # d loss / d softmax input, the form Softmax hands through
    net.Backpropagate(diff.to(dev))
    pieces.add(int(aslp.lib.aslp_lstm_seq_last_pieces()))
print(json.dumps({"losses": losses, "pieces": sorted(pieces), "planes": int(aslp.lib.aslp_gemm_operand_planes_get())}))
'''


def test_training_loss_stays_with_the_one_plane_mode(tmp_path):
    """7. 2 x LC-BLSTM + Affine + Softmax, 50 steps with momentum 0.9 from one initial model: default, ASLP_GEMM_PLANES=1 (fp16 operands in the
    layer products: the mode this one completes, same 11-bit rounding of the same kind of operand) and both switches.  The largest per-step
    loss gap of the combined mode to the default run may be at most 4 x that of ASLP_GEMM_PLANES=1 alone.  The net's widths are multiples of 64
    and a chunk is 128 rows, so that the layer products are ones the one-plane switch reaches (on a narrower net it changes no bit and the
    yardstick would be zero: asserted)."""
    def child(**env):
        p = subprocess.run([sys.executable, "-c", TRAIN_CHILD % {"root": ROOT}], env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        return json.loads(p.stdout.decode().strip().splitlines()[-1])
    base = child()
    planes = child(ASLP_GEMM_PLANES="1")
    both = child(ASLP_GEMM_PLANES="1", ASLP_LSTM_PIECES="1")
    assert base["pieces"] == [2] and base["planes"] == 2
    assert planes["pieces"] == [2] and planes["planes"] == 1          # under ASLP_GEMM_PLANES=1 alone the recurrences keep two pieces
    assert both["pieces"] == [1] and both["planes"] == 1
    l0, l1, l2 = (np.array(r["losses"]) for r in (base, planes, both))
    assert np.isfinite(l2).all() and l0[-5:].mean() < l0[:5].mean()     # the net does learn
    gap1, gap2 = float(np.abs(l1 - l0).max()), float(np.abs(l2 - l0).max())
    print("loss first / last: %.4f / %.4f; largest per-step loss gap to the default run: ASLP_GEMM_PLANES=1 %.3e, with ASLP_LSTM_PIECES=1 %.3e" % (l0[0], l0[-1], gap1, gap2))
    assert gap1 > 0.0, "ASLP_GEMM_PLANES=1 changed nothing on this net: the yardstick measures nothing"
    assert gap2 <= 4.0 * gap1, (gap1, gap2)


def test_long_sequence_hand_off(aslp, oracle, dev, tmp_path):
    """8. One LC-BLSTM layer at C = 512, R = 256, T = 300, S = 32 with a carried state, two chunks under one piece: 300 hand-offs per pass and
    direction -- a missed or stale piece anywhere in a chain shows in the last frames.  The library's error word stays clean and the last
    frame is within case 3's bound of the two-piece run."""
    marker, D, Cc, R, T, S = "<BLstmProjectedStreamsLC>", 40, 512, 256, 300, 32
    _, _, out_dim, path = build(oracle, tmp_path, marker, D, Cc, R, 5.0, seed=12, scale=0.05)
    two, pieces, paths = train_chunks(aslp, dev, path, marker, D, out_dim, T, S, chunk=T - 20)
    assert set(paths) == {PERSISTENT} and set(pieces) == {2}
    try:
        with aslp.ops.lstm_operand_pieces(1):
            one, pieces, paths = train_chunks(aslp, dev, path, marker, D, out_dim, T, S, chunk=T - 20)
    finally:
        aslp.ops.set_lstm_operand_pieces(-1)
    ok, msg = clean_error(aslp)
    assert ok, msg
    assert set(paths) == {PERSISTENT} and set(pieces) == {1}
    for k, (a, b) in enumerate(zip(one, two)):
        assert np.isfinite(a).all(), k
    for k in (0, 2):    # the outputs of the two chunks: last frame (forward direction's last hand-off) and first frame (backward direction's)
        a, b = one[k], two[k]
        print("T = 300 chunk %d: last frame %.3e, first frame %.3e, all frames %.3e" % (k // 2, rel(a[-S:], b[-S:]), rel(a[:S], b[:S]), rel(a, b)))
        assert rel(a[-S:], b[-S:]) < 1e-3 and rel(a[:S], b[:S]) < 1e-3
    for k in (1, 3):    # the in-diffs (printed: frame 0 is the end of the forward direction's BPTT chain)
        print("T = 300 chunk %d in-diff: first frame %.3e, last frame %.3e" % (k // 2, rel(one[k][:S], two[k][:S]), rel(one[k][-S:], two[k][-S:])))
