"""The recurrent layers on every path that is NOT the persistent kernel, against the oracle, with the path asserted.

A recurrent Propagate / Backpropagate runs on one of three sets of kernels (nnet/nnet-recurrent.cpp):
  persistent   one launch for all timesteps (csrc/rnn_persistent.hip): cells a multiple of 4 and at most 512, grid co-resident;
  step-fused   one fused launch per timestep (csrc/rnn_fused.hip lstm_step_fwd / lstm_step_bwd_gemm / lstm_step_bwd_cell,
               csrc/gru_fused.hip gru_step_*): cells a multiple of 4 where the persistent kernel does not apply -- every LSTM recipe of
               the reference (cell_dim 1024, recurrent_dim 512) -- or under ASLP_LSTM_PERSISTENT=0;
  unfused      a product and the cell kernels of csrc/rnn_cells.hip per timestep: any other cell count, or under ASLP_LSTM_UNFUSED=1.
The other recurrent tests run shapes the persistent kernel takes.  Here every case says which path it is meant for and asserts
aslp_recurrent_last_path() after both passes, so a change of dispatch cannot move a case onto other kernels unnoticed; and every case
compares Propagate output, input diff, updated parameters and the applied gradient tensor by tensor with the oracle chain of
test_rnn_gpu.py (same bars: relative error 1e-4, largest element 1e-3) over consecutive batches, so carried state, momentum and
the gradient clip are in play.

Shapes follow the step kernels' constants: 8 cells (x 4 gates) and 32 streams per forward workgroup, K = C split over 4 waves in
chunks of 8, the backward product's K = G C split over 8 workgroups x 4 waves."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nnet_io
from test_rnn_gpu import FAMILY, build, oracle_step

pytestmark = pytest.mark.gpu
TOL = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERSISTENT, STEP_FUSED, UNFUSED = 1, 2, 3   # aslp_recurrent_last_path (include/aslp_nnet.h)
PATH_NAME = {0: "none", PERSISTENT: "persistent", STEP_FUSED: "step-fused", UNFUSED: "unfused"}


def small(Cc):
    """parameter scale, gradient clip, learn rate, out-diff scale.  Under 100 cells the ragged small shapes' settings of test_rnn_gpu.py, from
    256 cells its C = 512 test's with the clip at 1 instead of 5; chosen so that the clip cuts some elements of the gradients and not most."""
    return (0.3, 0.5, 0.01, 1.0) if Cc < 100 else (0.2, 0.5, 0.01, 0.1) if Cc < 256 else (0.05, 1.0, 1e-3, 0.1)


def all_then_none(step, S, rng):
    return [1] * S if step == 0 else [0] * S


def mixed_resets(step, S, rng):
    """every stream starts fresh; from the second batch on some carry their state and some are reset (both kinds present when S > 1)"""
    if step == 0:
        return [1] * S
    flags = [int(v) for v in rng.integers(0, 2, S)]
    if S > 1:
        flags[0], flags[-1] = step % 2, 1 - step % 2
    return flags


def ragged_lengths(step, S, T, rng):
    """one stream of length T, one of length 1 (the masked branch from the second frame on), the rest anywhere between"""
    lens = rng.integers(1, T + 1, S).astype(np.int32)
    lens[0] = T
    if S > 1:
        lens[1] = 1
    return lens


def batch_plan(marker, dims, steps, seed, od_scale, resets, lengths, out_dim):
    """inputs, output diffs, reset flags / sequence lengths of every batch"""
    D, Cc, R, T, S = dims
    bidir, proj, cifg, lc, _ = FAMILY[marker]
    carried = (not bidir) or lc
    rng = np.random.default_rng(seed)
    plan = []
    for step in range(steps):
        x = rng.standard_normal((T * S, D)).astype(np.float32)
        od = (rng.standard_normal((T * S, out_dim)) * od_scale).astype(np.float32)
        flags = np.asarray(resets(step, S, rng), np.int32) if carried else None
        lens = None if carried else lengths(step, S, T, rng)
        plan.append((x, od, flags, lens))
    return plan


def oracle_steps(oracle, marker, dims, dirs, grads, plan, chunk, lr, mmt, clip):
    """The oracle chain over the batches of `plan`: per batch (output, input diff, parameters after, applied gradients by tensor)."""
    D, Cc, R, T, S = dims
    bidir, proj, cifg, lc, _ = FAMILY[marker]
    state = np.zeros((S, dirs[0].width), np.float32) if (not bidir) or lc else None
    ref = []
    for x, od, flags, lens in plan:
        if flags is not None:
            state[flags == 1] = 0
        out, idf, state = oracle_step(oracle, marker, dirs, grads, x, od, T, S, state, lens, chunk, lr, mmt, clip)
        ref.append((out, idf, np.concatenate([d.flat() for d in dirs]),
                    [(n, t.copy()) for di, g in enumerate(grads) for n, t in g.named_tensors("dir%d." % di)]))
    return ref


def compare(oracle, what, got, ref, lr):
    """got: per batch (output, input diff, parameters before, parameters after) of the engine; returns the largest errors seen"""
    worst = {}
    for step, ((out, idf, before, after), (out_ref, idf_ref, par_ref, grad_ref)) in enumerate(zip(got, ref)):
        for name, a, b in (("out", out, out_ref), ("in_diff", idf, idf_ref), ("params", after, par_ref)):
            assert a.shape == b.shape and np.isfinite(a).all(), (what, name, step)
            rel, mx = oracle.rel_err(a, b), oracle.max_err(a, b)
            assert rel < TOL and mx < 10 * TOL, (what, name, step, rel, mx)
            worst[name] = tuple(max(p) for p in zip(worst.get(name, (0.0, 0.0)), (rel, mx)))
        oracle.assert_applied_gradients(before, after, lr, grad_ref, TOL, (what, step))
    print("rnn-paths %s: relative / element error  " % (what,) + "  ".join("%s %.1e / %.1e" % ((k,) + v) for k, v in worst.items()))
    return worst


def run_lstm(aslp, oracle, dev, tmp_path, marker, dims, want, steps=2, seed=21, resets=all_then_none, lengths=ragged_lengths, lc_right=2):
    """`steps` consecutive training batches of one LSTM-family component on the engine and in the oracle; the recurrence must have run
    on the path `want`, forward and backward."""
    D, Cc, R, T, S = dims
    bidir, proj, cifg, lc, _ = FAMILY[marker]
    scale, clip, lr, od_scale = small(Cc)
    mmt = 0.9
    dirs, grads, out_dim, path = build(oracle, tmp_path, marker, D, Cc, R, clip, seed=seed, scale=scale)
    net = aslp.Nnet.Read(path)
    net.SetTrainOptions(learn_rate=lr, momentum=mmt)
    assert oracle.rel_err(net.GetParams(), np.concatenate([d.flat() for d in dirs])) == 0.0
    chunk = T - lc_right if lc else 0
    if lc:
        net.SetChunkSize(chunk)
    plan = batch_plan(marker, dims, steps, seed + 1, od_scale, resets, lengths, out_dim)
    ref = oracle_steps(oracle, marker, dims, dirs, grads, plan, chunk, lr, mmt, clip)
    got = []
    for step, (x, od, flags, lens) in enumerate(plan):
        if flags is not None:
            net.ResetLstmStreams([int(v) for v in flags])
        else:
            net.SetSeqLengths(lens)
        out = net.Propagate(torch.from_numpy(x).to(dev)).cpu().numpy()
        assert aslp.lib.aslp_recurrent_last_path(0) == want, (marker, dims, "forward ran", PATH_NAME[aslp.lib.aslp_recurrent_last_path(0)])
        before = net.GetParams()
        idf = net.Backpropagate(torch.from_numpy(od).to(dev), want_in_diff=True).cpu().numpy()
        assert aslp.lib.aslp_recurrent_last_path(1) == want, (marker, dims, "backward ran", PATH_NAME[aslp.lib.aslp_recurrent_last_path(1)])
        got.append((out, idf, before, net.GetParams()))
    return compare(oracle, "%s %s %s" % (PATH_NAME[want], marker, dims), got, ref, lr)


# ---- (a) the recipes' size (cell_dim 1024, recurrent_dim 512, 32 streams) on the per-timestep kernels -------------------------------

@pytest.mark.parametrize("marker", list(FAMILY))
def test_lstm_family_at_the_recipes_cell_dim_1024(aslp, oracle, dev, tmp_path, marker):
    """K = 1024 in lstm_step_fwd (32 chunks per wave), K = 4096 (3072 with coupled gates) in lstm_step_bwd_gemm, 128 cell blocks."""
    run_lstm(aslp, oracle, dev, tmp_path, marker, (64, 1024, 512, 12, 32), STEP_FUSED, lc_right=4)


def run_gru(aslp, oracle, dev, tmp_path, dims, want, steps=3):
    D, H, T, S = dims
    scale, clip, lr, od_scale = small(H)
    mmt = 0.9
    rng = np.random.default_rng(2)
    p, g = oracle.Gru(D, H, rng, scale=scale), oracle.Gru(D, H, zero=True)
    path = tmp_path / "gru.nnet"
    nnet_io.write_simple_nnet(path, [("<GruStreams>", D, H, nnet_io.gru(p, clip))])
    net = aslp.Nnet.Read(path)
    net.SetTrainOptions(learn_rate=lr, momentum=mmt)
    assert oracle.rel_err(net.GetParams(), p.flat()) == 0.0
    state = np.zeros((S, 5 * H), np.float32)
    got, ref = [], []
    for step in range(steps):
        x = rng.standard_normal((T * S, D)).astype(np.float32)
        od = (rng.standard_normal((T * S, H)) * od_scale).astype(np.float32)
        flags = mixed_resets(step, S, rng)
        net.ResetLstmStreams(flags)
        state[np.asarray(flags) == 1] = 0
        buf = p.forward(x, T, S, init_state=state)
        state = buf[T * S:(T + 1) * S].copy()
        dbuf, idf_ref = p.backward(od, T, S, buf)
        p.grads(g, x, T, S, buf, dbuf, mmt, clip)
        p.update(g, lr)
        ref.append((p.out_of(buf, T, S), idf_ref, p.flat(), [(n, getattr(g, n).copy()) for n in g.NAMES]))
        out = net.Propagate(torch.from_numpy(x).to(dev)).cpu().numpy()
        assert aslp.lib.aslp_recurrent_last_path(0) == want, (dims, "forward ran", PATH_NAME[aslp.lib.aslp_recurrent_last_path(0)])
        before = net.GetParams()
        idf = net.Backpropagate(torch.from_numpy(od).to(dev), want_in_diff=True).cpu().numpy()
        assert aslp.lib.aslp_recurrent_last_path(1) == want, (dims, "backward ran", PATH_NAME[aslp.lib.aslp_recurrent_last_path(1)])
        got.append((out, idf, before, net.GetParams()))
    return compare(oracle, "%s <GruStreams> %s" % (PATH_NAME[want], dims), got, ref, lr)


# (64, 1024, 8, 32): the recipes' width; (20, 1028, 4, 33): a last column block of 4 cells (gru_step_fwd1 owns 16, the others 32) and a
# second stream block holding one stream; (7, 6, 5, 3) / (33, 50, 7, 5) / (24, 1022, 4, 8): widths that only the unfused kernels take
@pytest.mark.parametrize("dims,want", [((64, 1024, 8, 32), STEP_FUSED), ((20, 1028, 4, 33), STEP_FUSED),
                                       ((7, 6, 5, 3), UNFUSED), ((33, 50, 7, 5), UNFUSED), ((24, 1022, 4, 8), UNFUSED)])
def test_gru_outside_the_persistent_kernel(aslp, oracle, dev, tmp_path, dims, want):
    run_gru(aslp, oracle, dev, tmp_path, dims, want)


# ---- (b) edges of rnn_fused.hip, all above 512 cells (no switch needed) ----------------------------------------------------------------

# C = 516: 65 forward K chunks (17 + 17 + 17 + 14 over the waves, half of the last chunk beyond K), a last workgroup of 4 cells, 258
#          backward chunks in 29 of the 32 parts (three parts empty);  C = 1020: 128 cell blocks, the last of 4 cells, 510 backward chunks
#          (the last part short), 383 with coupled gates (the last chunk half used);  C = 520: whole chunks, 65 of them.
# S = 1, 31: one stream block partly filled (rows clamped to S - 1);  33: a second block holding one stream;  70: three blocks.
# R = 0: W_eff is W_r itself;  R = 130: a projection width that is no multiple of 4.
EDGES = [
    ("<Lstm>", (20, 516, 0, 6, 33)),
    ("<BLstm>", (16, 1020, 0, 5, 4)),
    ("<LstmProjectedStreams>", (16, 516, 64, 5, 1)),
    ("<LstmProjectedStreams>", (24, 516, 260, 6, 31)),
    ("<LstmProjectedStreams>", (40, 1020, 510, 6, 8)),
    ("<BLstmProjectedStreams>", (24, 516, 128, 9, 6)),
    ("<BLstmProjectedStreams>", (24, 1020, 510, 5, 33)),
    ("<BLstmProjectedStreamsLC>", (24, 520, 130, 7, 70)),
    ("<LstmCifgProjectedStreams>", (40, 1020, 500, 6, 33)),
    ("<LstmCifgProjectedStreams>", (24, 516, 260, 5, 5)),
]


@pytest.mark.parametrize("marker,dims", EDGES)
def test_step_kernels_at_partial_blocks_and_ragged_k(aslp, oracle, dev, tmp_path, marker, dims):
    """Three batches: the carried-state members with mixed ResetLstmStreams flags on the second and third, the bidirectional
    non-LC members with ragged SetSeqLengths (one stream of length 1, one of length T: the `masked` branch of the step kernels)."""
    run_lstm(aslp, oracle, dev, tmp_path, marker, dims, STEP_FUSED, steps=3, seed=31, resets=mixed_resets)


def test_step_kernels_over_a_long_sequence(aslp, oracle, dev, tmp_path):
    """T = 80 launches per pass at the recipes' width, 8 streams, state carried into a second batch: an error that grows with every
    timestep shows in the last frames of the output and the first frames of the input diff.  (The oracle's share: about 1 s.)"""
    run_lstm(aslp, oracle, dev, tmp_path, "<LstmProjectedStreams>", (40, 1024, 512, 80, 8), STEP_FUSED, seed=41)


# ---- (c) the unfused path, reached by shape: cell counts that are no multiple of 4 -------------------------------------------------------

@pytest.mark.parametrize("marker", list(FAMILY))
@pytest.mark.parametrize("dims", [(7, 6, 3, 5, 3), (33, 50, 17, 9, 5), (40, 130, 66, 8, 33), (24, 1022, 510, 6, 8)])
def test_cell_kernels_when_cells_are_no_multiple_of_4(aslp, oracle, dev, tmp_path, marker, dims):
    run_lstm(aslp, oracle, dev, tmp_path, marker, dims, UNFUSED, steps=3, seed=51, resets=mixed_resets)


# ---- (d) the forced fall-backs at shapes the persistent kernel would take -------------------------------------------------------------------
# The switches are read once per process: one child process per (switch, shape), both markers in it, one child after another.  The child
# only drives the engine on files the parent wrote and writes back what it got; the parent compares with the oracle.

CHILD = r'''
import sys
import numpy as np, torch
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import aslp_import
aslp = aslp_import.load(); aslp.ops.use_torch_stream()
dev = torch.device("cuda:0")
work = sys.argv[1]
res = {}
for k in range(int(sys.argv[2])):
    job = np.load("%%s/job%%d.npz" %% (work, k))
    net = aslp.Nnet.Read("%%s/case%%d/rnn.nnet" %% (work, k))
    net.SetTrainOptions(learn_rate=float(job["lr"]), momentum=float(job["mmt"]))
    if int(job["chunk"]) > 0:
        net.SetChunkSize(int(job["chunk"]))
    paths = []
    for step in range(int(job["steps"])):
        if ("flags%%d" %% step) in job.files:
            net.ResetLstmStreams([int(v) for v in job["flags%%d" %% step]])
        else:
            net.SetSeqLengths(job["lens%%d" %% step])
        res["out%%d_%%d" %% (k, step)] = net.Propagate(torch.from_numpy(job["x%%d" %% step]).to(dev)).cpu().numpy()
        paths.append(aslp.lib.aslp_recurrent_last_path(0))
        res["before%%d_%%d" %% (k, step)] = np.asarray(net.GetParams(), np.float32)
        res["idf%%d_%%d" %% (k, step)] = net.Backpropagate(torch.from_numpy(job["od%%d" %% step]).to(dev), want_in_diff=True).cpu().numpy()
        paths.append(aslp.lib.aslp_recurrent_last_path(1))
        res["after%%d_%%d" %% (k, step)] = np.asarray(net.GetParams(), np.float32)
    res["paths%%d" %% k] = np.asarray(paths, np.int32)
np.savez(work + "/result.npz", **res)
'''

CHILD_MARKERS = ("<BLstmProjectedStreamsLC>", "<LstmCifgProjectedStreams>")
first_failed_child = []   # [(case id, what happened)]: once a child ended badly, no further child is started


@pytest.mark.parametrize("dims", [(64, 512, 256, 12, 32), (33, 48, 17, 9, 5)])
@pytest.mark.parametrize("switch,want", [("ASLP_LSTM_PERSISTENT=0", STEP_FUSED), ("ASLP_LSTM_UNFUSED=1", UNFUSED)])
def test_forced_fallbacks_match_oracle(oracle, dev, tmp_path, request, switch, want, dims):
    if first_failed_child:
        pytest.fail("not started: the child of %s ended badly, and nothing more runs on the GPU behind it\n%s" % first_failed_child[0])
    D, Cc, R, T, S = dims
    scale, clip, lr, od_scale = small(Cc)
    mmt, steps = 0.9, 2
    refs = []
    for k, marker in enumerate(CHILD_MARKERS):
        lc = FAMILY[marker][3]
        case = tmp_path / ("case%d" % k)
        case.mkdir()
        dirs, grads, out_dim, path = build(oracle, case, marker, D, Cc, R, clip, seed=61 + k, scale=scale)
        chunk = T - 4 if lc else 0
        plan = batch_plan(marker, dims, steps, 71 + k, od_scale, mixed_resets, ragged_lengths, out_dim)
        job = dict(lr=lr, mmt=mmt, chunk=chunk, steps=steps)
        for step, (x, od, flags, lens) in enumerate(plan):
            job.update({"x%d" % step: x, "od%d" % step: od})
            job.update({"flags%d" % step: flags} if flags is not None else {"lens%d" % step: lens})
        np.savez(tmp_path / ("job%d.npz" % k), **job)
        refs.append(oracle_steps(oracle, marker, dims, dirs, grads, plan, chunk, lr, mmt, clip))
    name, value = switch.split("=")
    try:
        # a fresh interpreter (the parent, which has the GPU open, is not replaced); the time limit covers its torch import on a cold machine
        p = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}, str(tmp_path), str(len(CHILD_MARKERS))], env=dict(os.environ, **{name: value}),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    except subprocess.TimeoutExpired as e:
        first_failed_child.append((request.node.name, "time limit of 300 s\n" + (e.stderr or b"").decode(errors="replace")[-2000:]))
        pytest.fail("child ran into its time limit")
    if p.returncode != 0:
        first_failed_child.append((request.node.name, "exit status %d\n%s" % (p.returncode, p.stderr.decode(errors="replace")[-2000:])))
        pytest.fail("child ended with status %d\n%s" % (p.returncode, p.stderr.decode(errors="replace")[-2000:]))
    res = np.load(tmp_path / "result.npz")
    for k, marker in enumerate(CHILD_MARKERS):
        assert [int(v) for v in res["paths%d" % k]] == [want] * (2 * steps), (switch, marker, dims, [PATH_NAME[int(v)] for v in res["paths%d" % k]])
        got = [tuple(res["%s%d_%d" % (n, k, step)] for n in ("out", "idf", "before", "after")) for step in range(steps)]
        compare(oracle, "%s %s %s %s" % (switch, PATH_NAME[want], marker, dims), got, refs[k], lr)
