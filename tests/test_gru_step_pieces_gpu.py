"""The opt-in fp16-piece products of the per-timestep GRU path (aslp_gru_step_pieces, ASLP_GRU_STEP_PIECES; csrc/gru_fused.hip
gru_step_fwd1_h / fwd2_h / bwd1_h / bwd2_h).

  1. direct, through the C ABI on padded buffers, against the float64 model of tests/gru_step_ref.py (pinned to the oracle on the CPU by
     tests/test_gru_step_ref_cpu.py), on gru_step_ref.SHAPES with has_next 1 and 0: two pieces at lstm_seq_ref.BAR (relative l2 1e-5,
     element 1e-4) against float64, one piece at those bars against the rounded-operand model and at BAR_ONE_PIECE (2e-3 / 2e-2) against
     the unrounded one; the padding's sentinel survives, two runs give the same bits, an all-zero [d_z | d_r] row adds an exact zero,
     aslp_gru_step_last_pieces() follows; too-short and misaligned planes are errors, not launches;
  2. through the engine: run_gru of tests/test_rnn_paths_gpu.py at its two step-path shapes, two pieces at that file's bars against the
     oracle chain, one piece against the two-piece run at BAR_ONE_PIECE;
  3. default untouched: with the switch at 0 the same shapes give the bits of a fresh process that never touched a new entry point, and
     ASLP_GRU_STEP_PIECES=1 turns the kernels on in a child.

Figures of the direct cases on an MI355X (worst over all cases and tensors; relative l2 / element):
  two pieces vs float64 1.5e-07 / 2.7e-07, the fp32-instruction kernels on the same inputs 1.9e-07 / 2.3e-07 (both are the fp32 gate
  arithmetic's own rounding), one piece vs the rounded-operand model 1.1e-06 / 1.0e-05 (the kernels split the fp32 g(t) and d_m(t) they
  stored, the model its float64 ones: a value next to an fp16 rounding boundary can fall either way), one piece vs float64 4.2e-04 / 5.9e-04.
Through the engine: two pieces vs the oracle chain out 3.4e-07 / 4.2e-07, in-diff 7.0e-07 / 6.7e-07 (H = 1024 / 1028); one piece vs the
two-piece run out 8.9e-05, in-diff 8.9e-05, parameters 7.4e-07."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gru_step_ref as ref
import nnet_io
from lstm_seq_ref import BAR, BAR_ONE_PIECE, CANARY
from test_rnn_paths_gpu import STEP_FUSED, ROOT, mixed_resets, run_gru, small

pytestmark = pytest.mark.gpu


# ---- 1. direct ------------------------------------------------------------------------------------------------------------------------------

class Direct:
    """Padded device buffers of one step; rows 1..S and columns [0, 5H) of every block are the data, the rest CANARY."""

    def __init__(self, aslp, dev, H, S):
        self.aslp, self.dev, self.H, self.S = aslp, dev, H, S
        self.W, self.ld = 5 * H, 5 * H + 8
        self.host = h = ref.step_inputs(H, S)
        t = self.devt = {n: self.block(h[n]) for n in ("y_prev", "y_next", "y_act", "y_x", "d_next", "d_cur")}
        t["w_zr"], t["w_m"] = self.padded(h["w_zr"]), self.padded(h["w_m"])
        t["w_zr_t"], t["w_m_t"] = self.padded(np.ascontiguousarray(h["w_zr"].T)), self.padded(np.ascontiguousarray(h["w_m"].T))
        self.planes = {n: aslp.ops.Planes(t[n][:, :t[n].shape[1] - 4]) for n in ("w_zr", "w_m", "w_zr_t", "w_m_t")}
        torch.cuda.synchronize()

    def block(self, a):
        buf = np.full((self.S + 2, self.ld), CANARY, np.float32)
        buf[1:self.S + 1, :self.W] = a
        return torch.from_numpy(buf).to(self.dev)

    def padded(self, a):
        buf = np.full((a.shape[0], a.shape[1] + 4), CANARY, np.float32)
        buf[:, :a.shape[1]] = a
        return torch.from_numpy(buf).to(self.dev)

    def planes_arg(self, backward):
        from kaldi_aslp_amd import _lib
        ph = _lib.GruStepH()
        for field, name in (("zr", "w_zr_t" if backward else "w_zr"), ("mg", "w_m_t" if backward else "w_m")):
            po = _lib.PlanesOut()
            self.aslp.lib.aslp_planes_as_output(self.planes[name].h, C.byref(po))
            setattr(ph, field + "_hi", po.hi), setattr(ph, field + "_lo", po.lo), setattr(ph, field + "_slot", po.slot), setattr(ph, "ldp_" + field, po.ld)
        return ph

    def forward(self, y_cur, ph):
        t, H = self.devt, self.H
        row1 = lambda x: x.data_ptr() + 4 * self.ld
        self.aslp.lib.aslp_gru_step_forward_h(row1(y_cur), row1(t["y_prev"]), t["w_zr"].data_ptr(), H + 4, t["w_m"].data_ptr(), H + 4, self.ld, self.S, H,
                                              C.byref(ph) if ph is not None else None)

    def backward(self, d_cur, ph, has_next):
        t, H = self.devt, self.H
        row1 = lambda x: x.data_ptr() + 4 * self.ld
        self.aslp.lib.aslp_gru_step_backward_h(row1(d_cur), row1(t["d_next"]), row1(t["y_act"]), row1(t["y_next"]), row1(t["y_prev"]), t["w_zr_t"].data_ptr(),
                                               2 * H + 4, t["w_m_t"].data_ptr(), H + 4, self.ld, self.S, H, int(has_next), C.byref(ph) if ph is not None else None)

    def run(self, pieces, has_next=True):
        """one forward and one backward step; returns (y_cur, d_cur) as host arrays, padding included"""
        aslp, t = self.aslp, self.devt
        y_cur, d_cur = t["y_x"].clone(), t["d_cur"].clone()
        keep = {n: v.clone() for n, v in t.items()}
        aslp.ops.set_gru_step_pieces(pieces)
        try:
            self.forward(y_cur, self.planes_arg(False))
            aslp.check_error()
            assert aslp.lib.aslp_gru_step_last_pieces() == pieces, ("forward", pieces)
            self.backward(d_cur, self.planes_arg(True), has_next)
            aslp.check_error()
            assert aslp.lib.aslp_gru_step_last_pieces() == pieces, ("backward", pieces)
            torch.cuda.synchronize()
        finally:
            aslp.ops.set_gru_step_pieces(-1)
        for n, v in keep.items():   # operands are read-only
            assert torch.equal(t[n], v), ("an operand changed", n)
        return y_cur.cpu().numpy(), d_cur.cpu().numpy()

    def check(self, got, want, bar, what):
        """every column block of both passes at (bar, 10 bar); the sentinel survives; returns the worst (l2, element)"""
        S, W = self.S, self.W
        for p, g in enumerate(got):
            assert np.isfinite(g[1:S + 1, :W]).all(), (what, p)
            pad = np.ones(g.shape, bool)
            pad[1:S + 1, :W] = False
            assert (g[pad] == np.float32(CANARY)).all(), (what, "pass", p, "padding written")
        worst = [0.0, 0.0]
        for name, (l2, el) in ref.step_errors([g[1:S + 1] for g in got], want, self.H).items():
            worst = [max(worst[0], l2), max(worst[1], el)]
            assert l2 < bar and el < 10 * bar, (what, name, l2, el)
        return tuple(worst)


figures = {}


@pytest.mark.parametrize("has_next", [1, 0])
@pytest.mark.parametrize("H,S", ref.SHAPES)
def test_step_kernels_against_float64(aslp, dev, H, S, has_next):
    case = Direct(aslp, dev, H, S)
    full, rounded1 = ref.step_model(case.host, 0, has_next), ref.step_model(case.host, 1, has_next)
    what = "H %d S %d has_next %d" % (H, S, has_next)
    two = case.run(2, has_next)
    e2 = case.check(two, full, BAR, what + " two pieces vs float64")
    again = case.run(2, has_next)
    assert all(np.array_equal(a, b) for a, b in zip(two, again)), (what, "two runs differ")
    e0 = case.check(case.run(0, has_next), full, 1.0, what + " fp32 instruction")   # printed, not held to a bar here (its own tests do that)
    one = case.run(1, has_next)
    e1r = case.check(one, rounded1, BAR, what + " one piece vs the rounded-operand model")
    e1 = case.check(one, full, BAR_ONE_PIECE, what + " one piece vs float64")
    assert all(np.array_equal(a, b) for a, b in zip(one, case.run(1, has_next))), (what, "two one-piece runs differ")
    assert not np.array_equal(one[0], two[0]) and not np.array_equal(one[1], two[1]), (what, "the piece count did not reach the kernels")
    print("gru-step %s: l2 / element  two pieces %.1e / %.1e  fp32 instruction %.1e / %.1e  one piece vs rounded model %.1e / %.1e  vs float64 %.1e / %.1e"
          % ((what,) + e2 + e0 + e1r + e1))
    for k, e in (("two", e2), ("fp32", e0), ("one_rounded", e1r), ("one", e1)):
        figures[k] = tuple(max(p) for p in zip(figures.get(k, (0.0, 0.0)), e))
    print("gru-step worst so far: " + "  ".join("%s %.1e / %.1e" % ((k,) + v) for k, v in figures.items()))
    if has_next:
        # the all-zero [d_z | d_r] row adds an exact zero: its whole diff row has the bits of the step that forms no first product
        zero = 1 + case.host["zero_row"]
        for pieces, got in ((2, two), (1, one)):
            without = case.run(pieces, False)
            assert np.array_equal(got[1][zero], without[1][zero]), (what, pieces, "all-zero row")
            assert S == 1 or not np.array_equal(got[1], without[1])


def test_bad_planes_are_an_error(aslp, dev):
    case = Direct(aslp, dev, 20, 5)
    y_cur, d_cur = case.devt["y_x"].clone(), case.devt["d_cur"].clone()
    aslp.ops.set_gru_step_pieces(2)
    try:
        def refused(call):
            call()
            with pytest.raises(RuntimeError, match="bad planes"):
                aslp.check_error()
        for field, value in (("ldp_zr", 16), ("ldp_mg", 16), ("ldp_zr", 68), ("zr_slot", None), ("mg_hi", None)):   # H = 20: K rounds up to 32
            ph = case.planes_arg(False)
            setattr(ph, field, value)
            refused(lambda: case.forward(y_cur, ph))
        ph = case.planes_arg(True)
        ph.ldp_zr = 32                                                          # backward: K = 2H = 40 rounds up to 48
        refused(lambda: case.backward(d_cur, ph, True))
        for field in ("zr_hi", "mg_lo"):                                        # misaligned planes
            ph = case.planes_arg(False)
            setattr(ph, field, getattr(ph, field) + 2)
            refused(lambda: case.forward(y_cur, ph))
        refused(lambda: case.forward(y_cur, None))
        aslp.ops.set_gru_step_pieces(1)                                         # one piece does not read lo: a missing lo plane is fine
        ph = case.planes_arg(False)
        ph.zr_lo = ph.mg_lo = None
        case.forward(y_cur.clone(), ph)
        aslp.check_error()
        torch.cuda.synchronize()
        assert torch.equal(y_cur, case.devt["y_x"]) and torch.equal(d_cur, case.devt["d_cur"])   # nothing was launched on the refused calls
    finally:
        aslp.ops.set_gru_step_pieces(-1)


# ---- 2. through the engine -----------------------------------------------------------------------------------------------------------------

ENGINE = [(64, 1024, 8, 32), (20, 1028, 4, 33)]   # the two step-path cases of test_rnn_paths_gpu.py: the recipes' width and the ragged one
STEPS = 2


def engine_inputs(oracle, tmp_path, dims):
    D, H, T, S = dims
    scale, clip, lr, od_scale = small(H)
    rng = np.random.default_rng(5)
    p = oracle.Gru(D, H, rng, scale=scale)
    path = tmp_path / "rnn.nnet"
    nnet_io.write_simple_nnet(path, [("<GruStreams>", D, H, nnet_io.gru(p, clip))])
    plan = []
    for step in range(STEPS):
        x = rng.standard_normal((T * S, D)).astype(np.float32)
        od = (rng.standard_normal((T * S, H)) * od_scale).astype(np.float32)
        plan.append((x, od, np.asarray(mixed_resets(step, S, rng), np.int32)))
    return str(path), plan, lr


def engine_run(aslp, dev, path, plan, lr, want_pieces):
    net = aslp.Nnet.Read(path)
    net.SetTrainOptions(learn_rate=lr, momentum=0.9)
    got = []
    for x, od, flags in plan:
        net.ResetLstmStreams([int(v) for v in flags])
        out = net.Propagate(torch.from_numpy(x).to(dev)).cpu().numpy()
        assert aslp.lib.aslp_recurrent_last_path(0) == STEP_FUSED and aslp.lib.aslp_gru_step_last_pieces() == want_pieces
        idf = net.Backpropagate(torch.from_numpy(od).to(dev), want_in_diff=True).cpu().numpy()
        assert aslp.lib.aslp_recurrent_last_path(1) == STEP_FUSED and aslp.lib.aslp_gru_step_last_pieces() == want_pieces
        got.append((out, idf, np.asarray(net.GetParams(), np.float32)))
    return got


@pytest.mark.parametrize("dims", ENGINE)
def test_engine_two_pieces_match_the_oracle_chain(aslp, oracle, dev, tmp_path, dims):
    """Three batches (momentum, clip, carried state, the planes re-made after every update) on the step-fused path, asserted in both passes
    by run_gru, at its bars against the oracle chain (relative 1e-4, element 1e-3)"""
    try:
        with aslp.ops.gru_step_pieces(2):
            run_gru(aslp, oracle, dev, tmp_path, dims, STEP_FUSED)
            assert aslp.lib.aslp_gru_step_last_pieces() == 2
    finally:
        aslp.ops.set_gru_step_pieces(-1)


@pytest.mark.parametrize("dims", ENGINE)
def test_engine_one_piece_stays_near_two_pieces(aslp, oracle, dev, tmp_path, dims):
    path, plan, lr = engine_inputs(oracle, tmp_path, dims)
    try:
        with aslp.ops.gru_step_pieces(2):
            two = engine_run(aslp, dev, path, plan, lr, 2)
        with aslp.ops.gru_step_pieces(1):
            one = engine_run(aslp, dev, path, plan, lr, 1)
    finally:
        aslp.ops.set_gru_step_pieces(-1)
    worst = {}
    for step, (a, b) in enumerate(zip(one, two)):
        for name, x, y in zip(("out", "in_diff", "params"), a, b):
            assert np.isfinite(x).all(), (dims, name, step)
            l2, el = oracle.rel_err(x, y), oracle.max_err(x, y)
            worst[name] = tuple(max(p) for p in zip(worst.get(name, (0.0, 0.0)), (l2, el)))
            assert l2 < BAR_ONE_PIECE and el < 10 * BAR_ONE_PIECE, (dims, name, step, l2, el)
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(one, two)), "one piece gave the bits of two: the piece count did not reach the kernels"
    print("gru-step engine %s one piece vs two: " % (dims,) + "  ".join("%s %.1e / %.1e" % ((k,) + v) for k, v in worst.items()))


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
    seen = []
    for step in range(int(job["steps"])):
        net.ResetLstmStreams([int(v) for v in job["flags%%d" %% step]])
        res["out%%d_%%d" %% (k, step)] = net.Propagate(torch.from_numpy(job["x%%d" %% step]).to(dev)).cpu().numpy()
        seen += [aslp.lib.aslp_recurrent_last_path(0), aslp.lib.aslp_gru_step_last_pieces() if %(probe)d else 0]
        res["idf%%d_%%d" %% (k, step)] = net.Backpropagate(torch.from_numpy(job["od%%d" %% step]).to(dev), want_in_diff=True).cpu().numpy()
        seen += [aslp.lib.aslp_recurrent_last_path(1), aslp.lib.aslp_gru_step_last_pieces() if %(probe)d else 0]
        res["after%%d_%%d" %% (k, step)] = np.asarray(net.GetParams(), np.float32)
    res["seen%%d" %% k] = np.asarray(seen, np.int32)
np.savez(work + "/result.npz", **res)
'''


def run_child(tmp_path, inputs, probe, **env):
    """the cases' batches through the engine in a fresh interpreter (the parent, which has the GPU open, is not replaced); probe 0: the child
    calls none of the new entry points itself"""
    for k, (path, plan, lr) in enumerate(inputs):
        job = dict(lr=lr, steps=len(plan))
        for step, (x, od, flags) in enumerate(plan):
            job.update({"x%d" % step: x, "od%d" % step: od, "flags%d" % step: flags})
        np.savez(tmp_path / ("job%d.npz" % k), **job)
    full = {k: v for k, v in os.environ.items() if k not in ("ASLP_GRU_STEP_PIECES", "ASLP_FP16_OPERANDS")}
    full.update(env)
    p = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "probe": probe}, str(tmp_path), str(len(inputs))], env=full, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, "child ended with status %d\n%s" % (p.returncode, p.stderr.decode(errors="replace")[-2000:])
    res = np.load(tmp_path / "result.npz")
    return [([tuple(res["%s%d_%d" % (n, k, step)] for n in ("out", "idf", "after")) for step in range(STEPS)], [int(v) for v in res["seen%d" % k]])
            for k in range(len(inputs))]


def prepare(oracle, tmp_path, cases):
    inputs = []
    for k, dims in enumerate(cases):
        case = tmp_path / ("case%d" % k)
        case.mkdir()
        inputs.append(engine_inputs(oracle, case, dims))
    return inputs


def same_bits(a, b):
    return all(np.array_equal(x, y) for sa, sb in zip(a, b) for x, y in zip(sa, sb))


def test_switch_off_gives_the_bits_of_a_process_that_never_touched_it(aslp, oracle, dev, tmp_path):
    inputs = prepare(oracle, tmp_path, ENGINE)
    aslp.ops.set_gru_step_pieces(1)    # this process has had the switch on (and the tests above ran the fp16 kernels in it)
    aslp.ops.set_gru_step_pieces(0)
    try:
        here = [engine_run(aslp, dev, *inp, 0) for inp in inputs]
    finally:
        aslp.ops.set_gru_step_pieces(-1)
    there = run_child(tmp_path, inputs, 0)
    for dims, h, (t, seen) in zip(ENGINE, here, there):
        assert seen == [STEP_FUSED, 0] * (2 * STEPS), (dims, seen)
        assert same_bits(h, t), (dims, "the switch-off run differs from a fresh process")


def test_environment_switch_turns_the_kernels_on_in_a_child(aslp, oracle, dev, tmp_path):
    cases = ENGINE[:1]   # the recipes' width
    inputs = prepare(oracle, tmp_path, cases)
    try:
        with aslp.ops.gru_step_pieces(1):
            here = engine_run(aslp, dev, *inputs[0], 1)
    finally:
        aslp.ops.set_gru_step_pieces(-1)
    (there, seen), = run_child(tmp_path, inputs, 1, ASLP_GRU_STEP_PIECES="1")
    assert seen == [STEP_FUSED, 1] * (2 * STEPS), seen
    assert same_bits(here, there), "the one-piece run is not reproducible from process to process"
