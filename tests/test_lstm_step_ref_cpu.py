"""CPU-only: what tests/test_lstm_step_split16_gpu.py stands on.
  * the float64 model of one step-fused LSTM timestep (tests/lstm_step_ref.py), unrounded, is pinned to the oracle (oracle/aslp_oracle_rnn.c)
    at the bars the persistent kernels' model is pinned at (tests/test_lstm_seq_ref_cpu.py), so the GPU tests do not compare the split-fp16
    step kernels with a model of themselves;
  * its operand rounding is what the contract of aslp_lstm_step_split16 says: 22 bits / fp16 behind power-of-two scales, the scales' extent;
  * the switch round-trips through the library, is off by default and follows ASLP_LSTM_STEP_SPLIT_F16;
  * kaldi-aslp_amd/_lib.py binds every new name with the header's layout."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import lstm_step_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-5   # relative l2 per tensor, 10 x that per element: tests/lstm_seq_ref.py BAR


# ---- the model against the oracle ------------------------------------------------------------------------------------------------------

def model_run(p, x, od, T, S, reverse, lens, state):
    """One direction of an oracle component, timestep by timestep through the model as the engine's step-fused branches drive the kernels:
    x-part + bias and dL/dm formed in float64 for all t, W_eff = W_r W_rm; with a projection and a carried state the first step's
    recurrent term is r(0) W_r^T, added by the caller (no_product)."""
    G, Cc, R = ref.gates(p.cifg), p.C, p.R
    W = (G + 3) * Cc
    om = (G + 2) * Cc
    f64 = lambda a: np.asarray(a, np.float64)
    y = np.zeros((T + 2, S, p.width))
    y[1:T + 1, :, :G * Cc] = (f64(x) @ f64(p.w_x).T + f64(p.bias)).reshape(T, S, G * Cc)
    if state is not None:
        y[T + 1 if reverse else 0] = state
    w_eff = f64(p.w_r) @ f64(p.w_rm) if R > 0 else f64(p.w_r)
    for step in range(T):
        t = T - step if reverse else 1 + step
        tp = t + 1 if reverse else t - 1
        first = step == 0 and R > 0 and state is not None
        if first:
            y[t, :, :G * Cc] += y[tp, :, W:W + R] @ f64(p.w_r).T
        y[t] = ref.forward(y[t], y[tp], w_eff, p.peep_i, p.peep_f, p.peep_o, p.cifg, masked=None if lens is None else t > lens, no_product=first)
        if R > 0:
            y[t, :, W:W + R] = y[t, :, om:om + Cc] @ f64(p.w_rm).T
    d = np.zeros((T + 2, S, p.width))
    d[1:T + 1, :, om:om + Cc] = (f64(od) @ f64(p.w_rm) if R > 0 else f64(od)).reshape(T, S, Cc)
    for step in range(T):
        t = 1 + step if reverse else T - step
        tn = t - 1 if reverse else t + 1
        tp = t + 1 if reverse else t - 1
        d[t] = ref.backward(d[t], d[tn], y[t], y[tn], y[tp], w_eff.T, p.peep_i, p.peep_f, p.peep_o, p.cifg, has_next=step > 0)
    return y, d


@pytest.mark.parametrize("marker,R,cifg,bidir", [("<Lstm>", 0, 0, 0), ("<BLstm>", 0, 0, 1), ("<LstmProjectedStreams>", 8, 0, 0),
                                                 ("<LstmCifgProjectedStreams>", 12, 1, 0)])
def test_model_matches_oracle(oracle, marker, R, cifg, bidir):
    """Two batches at C = 20, T = 6, S = 5; the unidirectional members carry their state into the second, <BLstm> masks its backward-in-time
    direction with ragged sequence lengths (0, 1, T - 1 and T among them).  The oracle's fp32 buffers against the float64 model."""
    D, Cc, T, S = 7, 20, 6, 5
    rng = np.random.default_rng(3)
    G = ref.gates(cifg)
    names = ["g"] + ([] if cifg else ["i"]) + ["f", "o", "c", "h", "m"]
    for reverse in range(2 if bidir else 1):
        p = oracle.LstmDir(D, Cc, R, cifg, rng, scale=0.3)
        state = None
        for batch in range(2):
            x = rng.standard_normal((T * S, D)).astype(np.float32)
            od = rng.standard_normal((T * S, p.rec)).astype(np.float32)
            lens = np.asarray([T, 0, 1, T - 1, 3], np.int32) if (bidir and reverse) else None
            buf = p.forward(x, T, S, reverse=bool(reverse), init_state=state, seq_len=lens)
            dbuf, _ = p.backward(od, T, S, buf, reverse=bool(reverse))
            y, d = model_run(p, x, od, T, S, reverse, lens, state)
            got_y, got_d = buf.reshape(T + 2, S, -1), dbuf.reshape(T + 2, S, -1)
            for what, g, r in (("y", got_y, y), ("d", got_d, d)):
                for k, name in enumerate(names):
                    l2, el = ref.errors(g[1:T + 1, :, k * Cc:(k + 1) * Cc], r[1:T + 1, :, k * Cc:(k + 1) * Cc])
                    assert l2 < BAR and el < 10 * BAR, (marker, "direction", reverse, "batch", batch, what, name, l2, el)
            if R > 0:
                l2, el = ref.errors(got_y[1:T + 1, :, (G + 3) * Cc:], y[1:T + 1, :, (G + 3) * Cc:])
                assert l2 < BAR and el < 10 * BAR, (marker, "r", l2, el)
            if lens is not None:
                assert not y[1:, 1].any() and not y[2:T + 1, 2].any() and y[1, 2].any() and not y[T, 3].any() and y[T - 1, 3].any()
            if not bidir:
                state = got_y[T].copy()


# ---- the operand rounding of the contract -------------------------------------------------------------------------------------------------

def test_operand_rounding_is_the_contracts():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((33, 300)) * np.exp(rng.uniform(-6, 2, (33, 1)))).astype(np.float32).astype(np.float64)
    assert ref.pow2_scale(0.0) == 1.0 and ref.pow2_scale(1.0) == 2.0 ** 13 and ref.pow2_scale(0.999) == 2.0 ** 14 and ref.pow2_scale(3.0) == 2.0 ** 12
    s = ref.pow2_scale(np.abs(x).max())
    assert 2.0 ** 13 <= np.abs(x).max() * s < 2.0 ** 14
    assert ref.round_pieces(x, 0) is not None and np.array_equal(ref.round_pieces(x, 0), x)
    two, one = ref.round_pieces(x, 2, s), ref.round_pieces(x, 1, s)
    big = np.abs(x * s) >= 2.0 ** -14   # fp16's normal range behind the scale
    assert np.max(np.abs(two - x)[big] / np.abs(x)[big]) <= 2.0 ** -22 and np.max(np.abs(two - x)) <= 2.0 ** -22 * np.abs(x).max()
    assert np.max(np.abs(one - x)[big] / np.abs(x)[big]) <= 2.0 ** -11
    assert np.array_equal(one, (x * s).astype(np.float16).astype(np.float64) / s)
    # m(t-1): no scale; the hi piece is fp16(m)
    m = np.tanh(rng.standard_normal(1000))
    assert np.array_equal(ref.round_pieces(m, 1), m.astype(np.float16).astype(np.float64))
    # dGATES: one scale per stream row and run of 128 consecutive k, counted from each K part's start; an all-zero row takes scale 1
    assert ref.dgates_runs(4096) == [(128 * k, 128 * (k + 1)) for k in range(32)]
    assert ref.dgates_runs(16) == [(0, 16)] and ref.dgates_runs(20) == [(0, 16), (16, 20)]
    runs = ref.dgates_runs(4 * 2048)
    assert len(runs) == 64 and runs[1] == (128, 256) and runs[-1] == (8064, 8192)
    runs = ref.dgates_runs(3 * 1020)   # 192 k steps over 32 parts of 6: every run is one part
    assert len(runs) == 32 and runs[0] == (0, 96) and runs[-1] == (2976, 3060)
    dg = x[:, :272].copy()
    dg[4] = 0
    dg[7, 128:256] *= 1e-6
    r1 = ref.dgates_operand(dg, 1)
    assert not r1[4].any()
    blk = dg[7:8, 128:256]
    assert np.array_equal(r1[7:8, 128:256], ref.round_pieces(blk, 1, ref.pow2_scale(np.abs(blk).max())))
    rel = np.abs(r1 - dg)[dg != 0] / np.abs(dg)[dg != 0]
    assert np.median(rel) < 2.0 ** -11 and ref.errors(ref.dgates_operand(dg, 2), dg)[0] < 2.0 ** -22
    # and through a step: the rounded-operand products stay within the one-piece / two-piece bars of the unrounded ones on benign inputs
    w = rng.uniform(-0.05, 0.05, (4 * 36, 36))
    full = ref.backward_product(dg[:, :144], w.T, False, 0)
    assert ref.errors(ref.backward_product(dg[:, :144], w.T, False, 2), full)[0] < 1e-6
    assert 1e-6 < ref.errors(ref.backward_product(dg[:, :144], w.T, False, 1), full)[0] < 2e-3


# ---- the switch ------------------------------------------------------------------------------------------------------------------------------

def test_switch_round_trips_and_is_off_by_default(aslp):
    lib, ops = aslp.lib, aslp.ops
    assert "ASLP_LSTM_STEP_SPLIT_F16" not in os.environ, "the suite runs with ASLP_LSTM_STEP_SPLIT_F16 unset"
    ops.set_lstm_step_split16(-1)
    assert lib.aslp_lstm_step_split16_get() == 0            # off by default
    try:
        ops.set_lstm_step_split16(1)
        assert lib.aslp_lstm_step_split16_get() == 1
        ops.set_lstm_step_split16(0)
        assert lib.aslp_lstm_step_split16_get() == 0
        with ops.lstm_step_split16(1):
            assert lib.aslp_lstm_step_split16_get() == 1
            with ops.lstm_step_split16(0):
                assert lib.aslp_lstm_step_split16_get() == 0
            assert lib.aslp_lstm_step_split16_get() == 1
        assert lib.aslp_lstm_step_split16_get() == 0
        with pytest.raises(RuntimeError):
            with ops.lstm_step_split16(1):
                raise RuntimeError("body")
        assert lib.aslp_lstm_step_split16_get() == 0            # restored although the body raised
        ops.set_lstm_step_split16(1)
        ops.set_lstm_step_split16(-1)
        assert lib.aslp_lstm_step_split16_get() == 0            # -1 hands the choice back to the (unset) environment
        # the piece count is the persistent kernels' own switch, untouched by this one
        before = lib.aslp_lstm_operand_pieces_get()
        with ops.lstm_step_split16(1):
            assert lib.aslp_lstm_operand_pieces_get() == before
        assert lib.aslp_lstm_step_last_pieces() == 0            # nothing launched on this thread
    finally:
        ops.set_lstm_step_split16(-1)


CHILD = r'''
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1], mode=ctypes.RTLD_GLOBAL)
lib.aslp_lstm_step_split16_get.restype = ctypes.c_int
a = lib.aslp_lstm_step_split16_get()
lib.aslp_lstm_step_split16(0); b = lib.aslp_lstm_step_split16_get()
lib.aslp_lstm_step_split16(-1); c = lib.aslp_lstm_step_split16_get()
print(a, b, c)
'''


@pytest.mark.parametrize("value,want", [("1", "1 0 1"), ("0", "0 0 0"), ("10", "0 0 0"), (None, "0 0 0")])
def test_environment_default(value, want):
    """a fresh process that only loads the library (no torch, no GPU): ASLP_LSTM_STEP_SPLIT_F16=1 turns the switch on, anything else leaves it off;
    an explicit setting wins and -1 hands the choice back"""
    from kaldi_aslp_amd import _lib
    env = {k: v for k, v in os.environ.items() if k != "ASLP_LSTM_STEP_SPLIT_F16"}
    if value is not None:
        env["ASLP_LSTM_STEP_SPLIT_F16"] = value
    p = subprocess.run([sys.executable, "-c", CHILD, _lib.LIB_PATH], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    assert p.stdout.decode().strip() == want


# ---- the binding ------------------------------------------------------------------------------------------------------------------------------

def test_lib_binds_every_new_name_with_the_headers_layout(aslp, tmp_path):
    from kaldi_aslp_amd import _lib
    sigs = {"aslp_lstm_step_split16": ([C.c_int], None), "aslp_lstm_step_split16_get": ([], C.c_int), "aslp_lstm_step_last_pieces": ([], C.c_int),
            "aslp_lstm_step_forward_h": ([C.POINTER(_lib.StepH)], None), "aslp_lstm_step_backward_h": ([C.POINTER(_lib.StepH)], None),
            "aslp_lstm_step_forward": ([C.POINTER(_lib.Step)], None), "aslp_lstm_step_backward": ([C.POINTER(_lib.Step)], None)}
    for name, (args, res) in sigs.items():
        fn = getattr(aslp.lib, name)
        assert list(fn.argtypes) == args and fn.restype is res, name
    assert callable(aslp.ops.set_lstm_step_split16) and callable(aslp.ops.lstm_step_split16)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "aslp_kernels.h"\nint main() { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(aslp_lstm_step_dir), sizeof(aslp_lstm_step), offsetof(aslp_lstm_step, ndir), offsetof(aslp_lstm_step_dir, seq_lengths), '
                   'sizeof(aslp_lstm_step_h), offsetof(aslp_lstm_step_h, w_hi), offsetof(aslp_lstm_step_h, w_slot), offsetof(aslp_lstm_step_h, ldp)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(v) for v in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE).stdout.split()]
    assert sizes == [C.sizeof(_lib.StepDir), C.sizeof(_lib.Step), _lib.Step.ndir.offset, _lib.StepDir.seq_lengths.offset, C.sizeof(_lib.StepH),
                     _lib.StepH.w_hi.offset, _lib.StepH.w_slot.offset, _lib.StepH.ldp.offset]
