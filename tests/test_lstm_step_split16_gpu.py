"""The opt-in split-fp16 products of the per-timestep LSTM path (aslp_lstm_step_split16, ASLP_LSTM_STEP_SPLIT_F16; csrc/rnn_fused.hip
lstm_step_fwd_h / lstm_step_bwd_gemm_h).

  1. direct, through the C ABI on padded buffers, against the float64 model of tests/lstm_step_ref.py (pinned to the oracle on the CPU by
     tests/test_lstm_step_ref_cpu.py): every k tail against the 16-wide k step, partial cell blocks of 8 (forward) and 32 (backward), a
     partial and a second stream block, both directions in one launch, coupled gates or not, a masked stream, no_product, has_next = 0;
     two pieces at the bars of the two-piece persistent kernels (tests/lstm_seq_ref.py BAR: relative l2 1e-5, element 1e-4), one piece at
     those bars against the rounded-operand model and at the one-piece bars (2e-3 / 2e-2) against the unrounded one; the padding's
     sentinel survives, two runs give the same bits, an all-zero dGATES row adds an exact zero, aslp_lstm_step_last_pieces() follows;
  2. through the engine: run_lstm of tests/test_rnn_paths_gpu.py with the switch on, at the recipes' size and at a ragged shape, on the
     step-fused path with two pieces at that file's bars against the oracle chain; one piece against the two-piece run;
  3. default untouched: with the switch off the same cases give the bits of a fresh process that never touched the switch, and
     ASLP_LSTM_STEP_SPLIT_F16=1 turns the kernels on in a child.

Figures of the direct cases on an MI355X (worst over all cases and tensors; relative l2 / element):
  two pieces vs float64 1.5e-07 / 2.8e-07, the fp32-instruction kernels on the same inputs 1.5e-07 / 2.9e-07 (both are the fp32 gate block's
  own rounding), one piece vs the rounded-operand model 1.7e-07 / 2.6e-07, one piece vs float64 3.2e-04 / 7.7e-04."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lstm_step_ref as ref
from lstm_seq_ref import BAR, BAR_ONE_PIECE, CANARY
from test_rnn_gpu import FAMILY, build
from test_rnn_paths_gpu import STEP_FUSED, PATH_NAME, ROOT, all_then_none, batch_plan, ragged_lengths, run_lstm, small

pytestmark = pytest.mark.gpu


# ---- 1. direct ------------------------------------------------------------------------------------------------------------------------------

T_NOW = 3   # the step's frame index, for the length masking


class Direct:
    """Padded device buffers of one step for two directions; rows 1..S and columns [0, W) of every block are the data, the rest CANARY."""

    def __init__(self, aslp, dev, Cc, S, cifg, seed, no_product=False, has_next=True):
        self.aslp, self.dev, self.C, self.S, self.cifg, self.no_product, self.has_next = aslp, dev, Cc, S, cifg, no_product, has_next
        G = self.G = ref.gates(cifg)
        self.W, self.ld, self.ldw_f, self.ldw_b = (G + 3) * Cc, (G + 3) * Cc + 8, Cc + 4, G * Cc + 4
        rng = np.random.default_rng(seed)
        og, oi, of, oo, oc, oh, om = ref.cols(Cc, cifg)
        self.host, self.devt, self.planes = [], [], []
        for d in range(2):
            h = {}
            act = lambda: np.concatenate([rng.uniform(-0.95, 0.95, (S, Cc)) if k in (og, oh, om) else rng.uniform(-2, 2, (S, Cc)) if k == oc
                                          else rng.uniform(0.05, 0.95, (S, Cc)) for k in range(0, self.W, Cc)], axis=1)
            h["y_prev"], h["y_next"], h["y_act"] = act(), act(), act()            # activations of the neighbours / of this step (backward)
            h["y_x"] = np.concatenate([rng.standard_normal((S, G * Cc)), np.zeros((S, 3 * Cc))], axis=1)   # forward: x-part + bias in the gate columns
            rows = np.exp(rng.uniform(np.log(1e-3), np.log(10.0), (S, 1)))
            h["d_next"] = rng.standard_normal((S, self.W)) * rows                    # rows of very different magnitude
            h["d_next"][S // 2 if d == 0 else 0, :G * Cc] = 0.0                      # an all-zero dGATES row
            h["d_cur"] = np.concatenate([np.zeros((S, (G + 2) * Cc)), rng.standard_normal((S, Cc))], axis=1)
            h["w"] = rng.uniform(-1, 1, (G * Cc, Cc)) * 0.5 / np.sqrt(Cc)            # W_eff; the backward pass reads its transpose
            for n in ("peep_i", "peep_f", "peep_o"):
                h[n] = rng.uniform(-0.3, 0.3, Cc)
            lens = np.full(S, T_NOW + 2, np.int32)
            if d == 1:
                lens[S - 1] = 1                                                     # the masked stream (direction 1 only, as in the engine)
                if S > 2:
                    lens[1] = T_NOW                                                 # t == length: still live
            h["lens"] = lens
            h = {k: (v.astype(np.float32) if v.dtype != np.int32 else v) for k, v in h.items()}
            self.host.append(h)
            t = {}
            for n in ("y_prev", "y_next", "y_act", "y_x", "d_next", "d_cur"):
                t[n] = self.block(h[n])
            t["w_f"], t["w_b"] = self.padded(h["w"], self.ldw_f), self.padded(np.ascontiguousarray(h["w"].T), self.ldw_b)
            for n in ("peep_i", "peep_f", "peep_o"):
                t[n] = torch.from_numpy(h[n]).to(dev)
            t["lens"] = torch.from_numpy(h["lens"]).to(dev)
            self.devt.append(t)
            self.planes.append((aslp.ops.Planes(t["w_f"][:, :Cc]), aslp.ops.Planes(t["w_b"][:, :G * Cc])))
        torch.cuda.synchronize()

    def block(self, a):
        buf = np.full((self.S + 2, self.ld), CANARY, np.float32)
        buf[1:self.S + 1, :self.W] = a
        return torch.from_numpy(buf).to(self.dev)

    def padded(self, a, ld):
        buf = np.full((a.shape[0], ld), CANARY, np.float32)
        buf[:, :a.shape[1]] = a
        return torch.from_numpy(buf).to(self.dev)

    def args(self, backward, y_cur, d_cur):
        from kaldi_aslp_amd import _lib
        ah = _lib.StepH()
        a = ah.step
        a.ndir, a.ld, a.ldw, a.S, a.C, a.cifg = 2, self.ld, self.ldw_b if backward else self.ldw_f, self.S, self.C, int(self.cifg)
        row1 = lambda t: t.data_ptr() + 4 * self.ld
        for d in range(2):
            t, q = self.devt[d], a.dir[d]
            q.y_cur, q.y_prev, q.y_next = row1(y_cur[d]), row1(t["y_prev"]), row1(t["y_next"])
            q.d_cur, q.d_next = row1(d_cur[d]), row1(t["d_next"])
            q.w = (t["w_b"] if backward else t["w_f"]).data_ptr()
            q.peep_i, q.peep_f, q.peep_o = (None if self.cifg else t["peep_i"].data_ptr()), t["peep_f"].data_ptr(), t["peep_o"].data_ptr()
            q.seq_lengths, q.t = (t["lens"].data_ptr() if d == 1 else None), T_NOW
            q.has_next, q.no_product = int(self.has_next), int(self.no_product and d == 0)
            po = _lib.PlanesOut()
            self.aslp.lib.aslp_planes_as_output(self.planes[d][1 if backward else 0].h, C.byref(po))
            ah.w_hi[d], ah.w_lo[d], ah.w_slot[d], ah.ldp = po.hi, po.lo, po.slot, po.ld
        return ah

    def run(self, split, pieces):
        """one forward and one backward launch; returns ([y_cur per direction], [d_cur per direction]) as host arrays, padding included"""
        aslp = self.aslp
        y_cur = [t["y_x"].clone() for t in self.devt]
        y_act = [t["y_act"].clone() for t in self.devt]
        d_cur = [t["d_cur"].clone() for t in self.devt]
        keep = [{n: t[n].clone() for n in ("y_prev", "y_next", "d_next", "w_f", "w_b")} for t in self.devt]
        aslp.ops.set_lstm_step_split16(split)
        aslp.ops.set_lstm_operand_pieces(pieces)
        try:
            want = 0 if split != 1 else (1 if pieces == 1 else 2)
            fa = self.args(False, y_cur, d_cur)
            aslp.lib.aslp_lstm_step_forward_h(C.byref(fa))
            aslp.check_error()
            assert aslp.lib.aslp_lstm_step_last_pieces() == want, ("forward", split, pieces)
            ba = self.args(True, y_act, d_cur)
            aslp.lib.aslp_lstm_step_backward_h(C.byref(ba))
            aslp.check_error()
            assert aslp.lib.aslp_lstm_step_last_pieces() == want, ("backward", split, pieces)
            torch.cuda.synchronize()
        finally:
            aslp.ops.set_lstm_step_split16(-1)
            aslp.ops.set_lstm_operand_pieces(-1)
        for d, t in enumerate(self.devt):   # operands are read-only
            for n, v in keep[d].items():
                assert torch.equal(t[n], v), ("an operand changed", d, n)
            assert torch.equal(y_act[d], t["y_act"])
        return [y.cpu().numpy() for y in y_cur], [dd.cpu().numpy() for dd in d_cur]

    def model(self, pieces):
        ys, ds = [], []
        for d, h in enumerate(self.host):
            masked = (T_NOW > h["lens"]) if d == 1 else None
            ys.append(ref.forward(h["y_x"], h["y_prev"], h["w"], h["peep_i"], h["peep_f"], h["peep_o"], self.cifg, masked=masked,
                                  no_product=self.no_product and d == 0, pieces=pieces))
            ds.append(ref.backward(h["d_cur"], h["d_next"], h["y_act"], h["y_next"], h["y_prev"], h["w"].T, h["peep_i"], h["peep_f"], h["peep_o"],
                                   self.cifg, has_next=self.has_next, pieces=pieces))
        return ys, ds

    def check(self, got, want, bar, what):
        """every column block of both passes and directions at (bar, 10 bar); the sentinel survives; returns the worst (l2, element)"""
        worst = [0.0, 0.0]
        names = ["g"] + ([] if self.cifg else ["i"]) + ["f", "o", "c", "h", "m"]
        for p, (gs, ws) in enumerate(zip(got, want)):
            for d in range(2):
                g = gs[d]
                assert np.isfinite(g[1:self.S + 1, :self.W]).all(), (what, p, d)
                pad = np.ones(g.shape, bool)
                pad[1:self.S + 1, :self.W] = False
                assert (g[pad] == np.float32(CANARY)).all(), (what, "pass", p, "direction", d, "padding written")
                for k, name in enumerate(names):
                    l2, el = ref.errors(g[1:self.S + 1, k * self.C:(k + 1) * self.C], ws[d][:, k * self.C:(k + 1) * self.C])
                    worst[0], worst[1] = max(worst[0], l2), max(worst[1], el)
                    assert l2 < bar and el < 10 * bar, (what, "pass", p, "direction", d, name, l2, el)
        return tuple(worst)


# C: 4 (one k step, a quarter used), 20 / 36 / 132 (k tails of 4; partial last cell blocks of 8 forward and of 32 backward; 132: 9 k steps
# over 4 waves, 33 / 25 over the backward's 32 parts);  S: 1, 31 (one partial stream block), 33 (a second block holding one stream)
DIRECT = [(Cc, S, (k + j) % 2) for k, Cc in enumerate((4, 20, 36, 132)) for j, S in enumerate((1, 31, 33))]
figures = {}


def direct_case(aslp, dev, Cc, S, cifg, **kw):
    case = Direct(aslp, dev, Cc, S, cifg, seed=100 + Cc + S, **kw)
    full, rounded1 = case.model(0), case.model(1)
    what = "C %d S %d cifg %d %s" % (Cc, S, cifg, kw or "")
    two = case.run(1, 2)
    e2 = case.check(two, full, BAR, what + " two pieces vs float64")
    again = case.run(1, 2)
    assert all(np.array_equal(a, b) for p in range(2) for a, b in zip(two[p], again[p])), (what, "two runs differ")
    e0 = case.check(case.run(0, 2), full, 1.0, what + " fp32 instruction")   # printed, not held to a bar here (its own tests do that)
    one = case.run(1, 1)
    e1r = case.check(one, rounded1, BAR, what + " one piece vs the rounded-operand model")
    e1 = case.check(one, full, BAR_ONE_PIECE, what + " one piece vs float64")
    print("lstm-step %s: l2 / element  two pieces %.1e / %.1e  fp32 instruction %.1e / %.1e  one piece vs rounded model %.1e / %.1e  vs float64 %.1e / %.1e"
          % ((what,) + e2 + e0 + e1r + e1))
    for k, e in (("two", e2), ("fp32", e0), ("one_rounded", e1r), ("one", e1)):
        figures[k] = tuple(max(p) for p in zip(figures.get(k, (0.0, 0.0)), e))
    print("lstm-step worst so far: " + "  ".join("%s %.1e / %.1e" % ((k,) + v) for k, v in figures.items()))
    return case, two, one


@pytest.mark.parametrize("Cc,S,cifg", DIRECT)
def test_step_kernels_against_float64(aslp, dev, Cc, S, cifg):
    case, two, one = direct_case(aslp, dev, Cc, S, cifg)
    G, om = case.G, (case.G + 2) * Cc
    for d, h in enumerate(case.host):
        zero = np.flatnonzero(~h["d_next"][:, :G * Cc].any(axis=1))
        assert zero.size >= 1
        for got in (two, one):   # d_m = dL/dm + 8 partial sums that are exactly zero: the bits of dL/dm
            assert np.array_equal(got[1][d][1 + zero, om:om + Cc], h["d_cur"][zero, om:om + Cc]), ("all-zero dGATES row", d)
        if d == 1:               # the masked stream: every column of the forward step is zero
            assert not two[0][d][S, :case.W].any() and not one[0][d][S, :case.W].any()
            assert S == 1 or two[0][d][1, :case.W].any()


@pytest.mark.parametrize("Cc,S,cifg", [(20, 33, 0), (132, 31, 1)])
def test_no_product_and_first_backward_step(aslp, dev, Cc, S, cifg):
    """no_product (direction 0 only: the other direction of the same launch still multiplies) and has_next = 0 (no product launch, the m
    columns of the diff stay as they came)"""
    case, two, one = direct_case(aslp, dev, Cc, S, cifg, no_product=True, has_next=False)
    om = (case.G + 2) * Cc
    for d, h in enumerate(case.host):
        assert np.array_equal(two[1][d][1:S + 1, om:om + Cc], h["d_cur"][:, om:om + Cc])
    # without a product the fp16 kernels compute what the fp32 ones do, bit for bit, in direction 0
    off = case.run(0, 2)
    assert np.array_equal(two[0][0], off[0][0]) and np.array_equal(one[0][0], off[0][0])
    assert not np.array_equal(two[0][1], one[0][1])


def test_bad_planes_are_an_error(aslp, dev):
    case = Direct(aslp, dev, 20, 5, 0, seed=1)
    y_cur = [t["y_x"].clone() for t in case.devt]
    d_cur = [t["d_cur"].clone() for t in case.devt]
    aslp.ops.set_lstm_step_split16(1)
    try:
        for field, value in (("ldp", 16), ("ldp", 68)):
            a = case.args(False, y_cur, d_cur)
            setattr(a, field, value)
            aslp.lib.aslp_lstm_step_forward_h(C.byref(a))
            with pytest.raises(RuntimeError, match="bad planes"):
                aslp.check_error()
        a = case.args(False, y_cur, d_cur)
        a.w_hi[1] = None
        aslp.lib.aslp_lstm_step_forward_h(C.byref(a))
        with pytest.raises(RuntimeError, match="bad planes"):
            aslp.check_error()
        torch.cuda.synchronize()
        assert all(torch.equal(y, t["y_x"]) for y, t in zip(y_cur, case.devt))   # nothing was launched
    finally:
        aslp.ops.set_lstm_step_split16(-1)


# ---- 2. through the engine -----------------------------------------------------------------------------------------------------------------

RECIPE = (64, 1024, 512, 12, 32)
ENGINE = [("<LstmProjectedStreams>", RECIPE), ("<BLstmProjectedStreamsLC>", RECIPE),
          # ragged: C = 516 (33 k steps, the last a quarter used; a last cell block of 4), a partial / a second stream block, R no multiple of 64
          ("<LstmProjectedStreams>", (24, 516, 260, 5, 31)), ("<BLstmProjectedStreamsLC>", (24, 516, 132, 6, 33))]
SEED, LC_RIGHT, STEPS = 21, 2, 2


def engine_inputs(oracle, tmp_path, marker, dims):
    """the model file and the batches run_lstm makes for these arguments"""
    D, Cc, R, T, S = dims
    scale, clip, lr, od_scale = small(Cc)
    dirs, grads, out_dim, path = build(oracle, tmp_path, marker, D, Cc, R, clip, seed=SEED, scale=scale)
    plan = batch_plan(marker, dims, STEPS, SEED + 1, od_scale, all_then_none, ragged_lengths, out_dim)
    return path, plan, lr, (T - LC_RIGHT if FAMILY[marker][3] else 0)


def engine_run(aslp, dev, path, plan, lr, chunk, want_pieces):
    net = aslp.Nnet.Read(path)
    net.SetTrainOptions(learn_rate=lr, momentum=0.9)
    if chunk:
        net.SetChunkSize(chunk)
    got = []
    for x, od, flags, lens in plan:
        if flags is not None:
            net.ResetLstmStreams([int(v) for v in flags])
        else:
            net.SetSeqLengths(lens)
        out = net.Propagate(torch.from_numpy(x).to(dev)).cpu().numpy()
        assert aslp.lib.aslp_recurrent_last_path(0) == STEP_FUSED and aslp.lib.aslp_lstm_step_last_pieces() == want_pieces
        idf = net.Backpropagate(torch.from_numpy(od).to(dev), want_in_diff=True).cpu().numpy()
        assert aslp.lib.aslp_recurrent_last_path(1) == STEP_FUSED and aslp.lib.aslp_lstm_step_last_pieces() == want_pieces
        got.append((out, idf, np.asarray(net.GetParams(), np.float32)))
    return got


@pytest.mark.parametrize("marker,dims", ENGINE)
def test_engine_two_pieces_match_the_oracle_chain(aslp, oracle, dev, tmp_path, marker, dims):
    """Two batches (momentum, clip, carried state, the planes re-made after the update) on the step-fused path, asserted in both passes by
    run_lstm, at its bars against the oracle chain (relative 1e-4, element 1e-3)"""
    try:
        with aslp.ops.lstm_step_split16(1), aslp.ops.lstm_operand_pieces(2):
            run_lstm(aslp, oracle, dev, tmp_path, marker, dims, STEP_FUSED, steps=STEPS, seed=SEED, lc_right=LC_RIGHT)
            assert aslp.lib.aslp_lstm_step_last_pieces() == 2
    finally:
        aslp.ops.set_lstm_step_split16(-1)
        aslp.ops.set_lstm_operand_pieces(-1)


@pytest.mark.parametrize("marker,dims", ENGINE)
def test_engine_one_piece_stays_near_two_pieces(aslp, oracle, dev, tmp_path, marker, dims):
    path, plan, lr, chunk = engine_inputs(oracle, tmp_path, marker, dims)
    try:
        with aslp.ops.lstm_step_split16(1):
            with aslp.ops.lstm_operand_pieces(2):
                two = engine_run(aslp, dev, path, plan, lr, chunk, 2)
            with aslp.ops.lstm_operand_pieces(1):
                one = engine_run(aslp, dev, path, plan, lr, chunk, 1)
    finally:
        aslp.ops.set_lstm_step_split16(-1)
        aslp.ops.set_lstm_operand_pieces(-1)
    worst = {}
    for step, (a, b) in enumerate(zip(one, two)):
        for name, x, y in zip(("out", "in_diff", "params"), a, b):
            assert np.isfinite(x).all(), (marker, dims, name, step)
            l2, el = oracle.rel_err(x, y), oracle.max_err(x, y)
            worst[name] = tuple(max(p) for p in zip(worst.get(name, (0.0, 0.0)), (l2, el)))
            assert l2 < BAR_ONE_PIECE and el < 10 * BAR_ONE_PIECE, (marker, dims, name, step, l2, el)
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(one, two)), "one piece gave the bits of two: the piece count did not reach the kernels"
    print("lstm-step engine %s %s one piece vs two: " % (marker, dims) + "  ".join("%s %.1e / %.1e" % ((k,) + v) for k, v in worst.items()))


# ---- 3. default untouched --------------------------------------------------------------------------------------------------------------------

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
    net.SetTrainOptions(learn_rate=float(job["lr"]), momentum=0.9)
    if int(job["chunk"]) > 0:
        net.SetChunkSize(int(job["chunk"]))
    seen = []
    for step in range(int(job["steps"])):
        if ("flags%%d" %% step) in job.files:
            net.ResetLstmStreams([int(v) for v in job["flags%%d" %% step]])
        else:
            net.SetSeqLengths(job["lens%%d" %% step])
        res["out%%d_%%d" %% (k, step)] = net.Propagate(torch.from_numpy(job["x%%d" %% step]).to(dev)).cpu().numpy()
        seen += [aslp.lib.aslp_recurrent_last_path(0), aslp.lib.aslp_lstm_step_last_pieces()]
        res["idf%%d_%%d" %% (k, step)] = net.Backpropagate(torch.from_numpy(job["od%%d" %% step]).to(dev), want_in_diff=True).cpu().numpy()
        seen += [aslp.lib.aslp_recurrent_last_path(1), aslp.lib.aslp_lstm_step_last_pieces()]
        res["after%%d_%%d" %% (k, step)] = np.asarray(net.GetParams(), np.float32)
    res["seen%%d" %% k] = np.asarray(seen, np.int32)
np.savez(work + "/result.npz", **res)
'''


def run_child(tmp_path, cases, inputs, **env):
    """the cases' batches through the engine in a fresh interpreter (the parent, which has the GPU open, is not replaced)"""
    for k, (path, plan, lr, chunk) in enumerate(inputs):
        job = dict(lr=lr, chunk=chunk, steps=len(plan))
        for step, (x, od, flags, lens) in enumerate(plan):
            job.update({"x%d" % step: x, "od%d" % step: od})
            job.update({"flags%d" % step: flags} if flags is not None else {"lens%d" % step: lens})
        np.savez(tmp_path / ("job%d.npz" % k), **job)
    full = {k: v for k, v in os.environ.items() if k != "ASLP_LSTM_STEP_SPLIT_F16"}
    full.update(env)
    p = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}, str(tmp_path), str(len(cases))], env=full, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, "child ended with status %d\n%s" % (p.returncode, p.stderr.decode(errors="replace")[-2000:])
    res = np.load(tmp_path / "result.npz")
    return [([tuple(res["%s%d_%d" % (n, k, step)] for n in ("out", "idf", "after")) for step in range(STEPS)], [int(v) for v in res["seen%d" % k]])
            for k in range(len(cases))]


def prepare(oracle, tmp_path, cases):
    inputs = []
    for k, (marker, dims) in enumerate(cases):
        case = tmp_path / ("case%d" % k)
        case.mkdir()
        inputs.append(engine_inputs(oracle, case, marker, dims))
    return inputs


def same_bits(a, b):
    return all(np.array_equal(x, y) for sa, sb in zip(a, b) for x, y in zip(sa, sb))


def test_switch_off_gives_the_bits_of_a_process_that_never_touched_it(aslp, oracle, dev, tmp_path):
    inputs = prepare(oracle, tmp_path, ENGINE)
    aslp.ops.set_lstm_step_split16(1)    # this process has had the switch on (and the tests above ran the fp16 kernels in it)
    aslp.ops.set_lstm_step_split16(0)
    try:
        with aslp.ops.lstm_operand_pieces(1):   # ... and the piece count keeps having no effect on this path
            here = [engine_run(aslp, dev, *inp, 0) for inp in inputs]
        assert aslp.lib.aslp_lstm_step_last_pieces() == 0
    finally:
        aslp.ops.set_lstm_step_split16(-1)
        aslp.ops.set_lstm_operand_pieces(-1)
    there = run_child(tmp_path, ENGINE, inputs)
    for (marker, dims), h, (t, seen) in zip(ENGINE, here, there):
        assert seen == [STEP_FUSED, 0] * (2 * STEPS), (marker, dims, seen)
        assert same_bits(h, t), (marker, dims, "the switch-off run differs from a fresh process")


def test_environment_switch_turns_the_kernels_on_in_a_child(aslp, oracle, dev, tmp_path):
    cases = ENGINE[:1]   # the recipes' size
    inputs = prepare(oracle, tmp_path, cases)
    try:
        with aslp.ops.lstm_step_split16(1), aslp.ops.lstm_operand_pieces(2):
            here = engine_run(aslp, dev, *inputs[0], 2)
    finally:
        aslp.ops.set_lstm_step_split16(-1)
        aslp.ops.set_lstm_operand_pieces(-1)
    (there, seen), = run_child(tmp_path, cases, inputs, ASLP_LSTM_STEP_SPLIT_F16="1")
    assert seen == [STEP_FUSED, 2] * (2 * STEPS), seen
    assert same_bits(here, there), "the two-piece run is not reproducible from process to process"
