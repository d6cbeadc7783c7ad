"""CPU-only: what tests/test_gru_step_pieces_gpu.py stands on.
  * T steps of the float64 model of one GRU timestep (tests/gru_step_ref.py) are the recurrence of tests/gru_seq_ref.py (1e-12) and the
    oracle's GRU (orc_gru_forward / orc_gru_backward, 5e-6), on T = 3, S = 3, H = 8;
  * its operand rounding is what the contract of aslp_gru_step_pieces says: the runs one backward scale covers, restated from the kernels'
    K split;
  * on the inputs of the direct GPU cases the rounded-operand model's own distance to the unrounded one stays inside the bars used there:
    two pieces inside BAR (1e-5 relative l2, 1e-4 element), one piece inside BAR_ONE_PIECE (2e-3 / 2e-2) -- and one piece does differ.
    Worst over all shapes, both has_next and all tensors: two pieces 9.5e-08 / 1.2e-07, one piece 4.2e-04 / 5.9e-04 (WORST below);
  * the binding declares the new entry points and the struct has the header's layout."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import gru_seq_ref
import gru_step_ref as ref
from lstm_seq_ref import BAR, BAR_ONE_PIECE

PIN = gru_seq_ref.Case(8, 3, 3, 1, ())
WORST = {2: (9.5e-08, 1.2e-07), 1: (4.2e-04, 5.9e-04)}   # as printed by test_rounded_model_stays_inside_the_bars_on_the_gpu_cases


def close(got, want, bar, what):
    l2, el = ref.errors(got, want)
    assert l2 < bar and el < bar, (what, l2, el)


def test_steps_are_the_sequence_model():
    inp = gru_seq_ref.build_case(PIN)
    ry, rd = gru_seq_ref.reference(inp)
    y, d = ref.recurrence(inp)
    H, T = PIN.H, PIN.T
    for k, name in enumerate(ref.NAMES):
        close(y[1:T + 1, :, k * H:(k + 1) * H], ry[1:T + 1, :, k * H:(k + 1) * H], 1e-12, name)
        close(d[1:T + 1, :, k * H:(k + 1) * H], rd[1:T + 1, :, k * H:(k + 1) * H], 1e-12, "d_" + name)
    assert np.abs(rd[1:T + 1]).min() > 0 and np.abs(ry[1:T + 1]).min() > 0


def test_steps_are_the_oracles_gru(oracle):
    D, H, S, T = 7, PIN.H, PIN.S, PIN.T
    rng = np.random.default_rng(17)
    p = oracle.Gru(D, H, rng, scale=0.3)
    x = rng.standard_normal((T * S, D)).astype(np.float32)
    od = rng.standard_normal((T * S, H)).astype(np.float32)
    state = np.zeros((S, 5 * H), np.float32)
    state[:, 4 * H:] = rng.standard_normal((S, H)).astype(np.float32) * 0.5
    buf = p.forward(x, T, S, init_state=state)
    dbuf, _ = p.backward(od, T, S, buf)
    f64 = lambda a: np.asarray(a, np.float64)
    y = np.zeros((T + 2, S, 5 * H))
    y[1:T + 1, :, :3 * H] = (f64(x) @ f64(p.w_zrm_x).T + f64(p.bias)).reshape(T, S, 3 * H)
    y[0] = state
    d = np.zeros((T + 2, S, 5 * H))
    d[1:T + 1, :, 4 * H:] = f64(od).reshape(T, S, H)
    my, md = ref.recurrence(dict(case=PIN, y=y, d=d, w_zr=p.w_zr_h, w_m=p.w_m_g))
    oy, od_ = buf.reshape(T + 2, S, -1), dbuf.reshape(T + 2, S, -1)
    for k, name in enumerate(ref.NAMES):
        close(oy[1:T + 1, :, k * H:(k + 1) * H], my[1:T + 1, :, k * H:(k + 1) * H], 5e-6, name)
        close(od_[1:T + 1, :, k * H:(k + 1) * H], md[1:T + 1, :, k * H:(k + 1) * H], 5e-6, "d_" + name)


def test_runs_follow_the_kernels_k_split():
    """K = 2 * 1024: 128 k steps, 32 per wave, four runs of 8 each -- 16 runs of 128 k; K = 264 (H = 132, first backward product): 17 k
    steps, 5 per wave, the last wave's slice 2 steps of which the second holds 8 k; K = 4: one run of 4 k in wave 0, none elsewhere"""
    assert ref.diff_runs(2048) == [(128 * i, 128 * (i + 1)) for i in range(16)]
    assert ref.diff_runs(264) == [(0, 80), (80, 160), (160, 240), (240, 264)]
    assert ref.diff_runs(4) == [(0, 4)]
    for K in (4, 8, 20, 36, 40, 72, 132, 264, 1024, 1028, 2056):
        runs = ref.diff_runs(K)
        assert runs[0][0] == 0 and runs[-1][1] == K and all(a[1] == b[0] and a[0] < a[1] <= a[0] + 128 for a, b in zip(runs, runs[1:] + [(K, K)]))


def test_diff_operand_scales_per_row_and_run():
    rng = np.random.default_rng(3)
    dx = rng.standard_normal((5, 264)) * np.exp(rng.uniform(-7, 2, (5, 1)))
    dx[2] = 0.0
    dx[3, 80:160] *= 2.0 ** 20            # a run of its own scale: the neighbours keep their precision
    one, two = ref.diff_operand(dx, 1), ref.diff_operand(dx, 2)
    assert not one[2].any() and not two[2].any()
    rel = lambda a: np.abs(a - dx)[dx != 0] / np.abs(dx)[dx != 0]
    assert rel(two).max() < 2.0 ** -19 and 2.0 ** -14 < rel(one).max() < 2.0 ** -5
    assert np.array_equal(ref.diff_operand(dx, 0), dx)
    # a power-of-two factor on a row changes nothing but the scale
    assert np.array_equal(ref.diff_operand(dx * 2.0 ** -9, 1), one * 2.0 ** -9)
    # within a run small values lose against the run's largest: fp16 spacing at the scaled maximum's exponent is the floor
    row = np.zeros((1, 16))
    row[0, 0], row[0, 1] = 1.0, 2.0 ** -40
    assert ref.diff_operand(row, 1)[0, 1] == 0.0 and ref.diff_operand(row, 2)[0, 1] == 2.0 ** -40   # (the lo' piece reaches 2^11 further down)


@pytest.mark.parametrize("H,S", ref.SHAPES)
def test_inputs_are_what_the_issue_names(H, S):
    h = ref.step_inputs(H, S)
    assert h["w_zr"].shape == (2 * H, H) and h["w_m"].shape == (H, H) and np.abs(h["w_zr"]).max() <= 0.5 / np.sqrt(H)
    assert all(h[n].shape == (S, 5 * H) and h[n].dtype == np.float32 for n in ("y_prev", "y_next", "y_act", "y_x", "d_next", "d_cur"))
    assert np.abs(h["y_prev"]).max() < 1 and h["y_prev"][:, :2 * H].min() > 0
    zero = np.flatnonzero(~h["d_next"][:, :2 * H].any(axis=1))
    assert list(zero) == [h["zero_row"]] and h["d_next"][h["zero_row"], 2 * H:].any()


def test_rounded_model_stays_inside_the_bars_on_the_gpu_cases():
    assert (BAR, BAR_ONE_PIECE) == (1e-5, 2e-3)
    worst = {1: [0.0, 0.0], 2: [0.0, 0.0]}
    for H, S in ref.SHAPES:
        h = ref.step_inputs(H, S)
        for has_next in (True, False):
            full = ref.step_model(h, 0, has_next)
            for pieces, bar in ((2, BAR), (1, BAR_ONE_PIECE)):
                got = ref.step_model(h, pieces, has_next)
                for name, (l2, el) in ref.step_errors(got, full, H).items():
                    assert l2 < bar and el < 10 * bar, (H, S, has_next, pieces, name, l2, el)
                    worst[pieces] = [max(worst[pieces][0], l2), max(worst[pieces][1], el)]
                if pieces == 1:
                    assert not np.array_equal(got[0], full[0]) and not np.array_equal(got[1], full[1]), (H, S, "one piece changed nothing")
    print("gru-step d_model worst (relative l2 / element): two pieces %.1e / %.1e, one piece %.1e / %.1e" % tuple(worst[2] + worst[1]))
    for pieces in (1, 2):
        assert worst[pieces][0] <= 1.05 * WORST[pieces][0] and worst[pieces][1] <= 1.05 * WORST[pieces][1], "the docstring's figures are stale"


# ---- the binding ------------------------------------------------------------------------------------------------------------------------------

def test_binding_declares_the_entry_points(aslp):
    C = ctypes
    i, vp = C.c_int, C.c_void_p
    hp = C.POINTER(aslp._lib.GruStepH)
    sigs = {"aslp_gru_step_pieces": ([i], None), "aslp_gru_step_pieces_get": ([], i), "aslp_gru_step_last_pieces": ([], i),
            "aslp_gru_step_forward_h": ([vp, vp, vp, i, vp, i, i, i, i, hp], None),
            "aslp_gru_step_backward_h": ([vp, vp, vp, vp, vp, vp, i, vp, i, i, i, i, i, hp], None),
            "aslp_fp16_operands": ([i], None), "aslp_fp16_operands_get": ([], i)}
    for name, (args, res) in sigs.items():
        fn = getattr(aslp.lib, name)
        assert list(fn.argtypes) == args and fn.restype is res, name
    assert all(callable(getattr(aslp.ops, n)) for n in ("set_gru_step_pieces", "gru_step_pieces", "set_fp16_operands", "fp16_operands"))
    assert aslp.lib.aslp_gru_step_last_pieces() == 0    # nothing launched on this thread


def test_struct_layout_is_the_headers(aslp, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "aslp_kernels.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", '
                   'sizeof(aslp_gru_step_h), offsetof(aslp_gru_step_h, zr_slot), offsetof(aslp_gru_step_h, mg_hi), offsetof(aslp_gru_step_h, ldp_zr), '
                   'offsetof(aslp_gru_step_h, ldp_mg)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE).stdout.split()]
    S = aslp._lib.GruStepH
    assert got == [ctypes.sizeof(S), S.zr_slot.offset, S.mg_hi.offset, S.ldp_zr.offset, S.ldp_mg.offset]


def test_switch_roundtrip(aslp):
    lib, ops = aslp.lib, aslp.ops
    ops.set_gru_step_pieces(-1)
    assert lib.aslp_gru_step_pieces_get() == 0            # off by default
    try:
        for n in (1, 2, 0):
            ops.set_gru_step_pieces(n)
            assert lib.aslp_gru_step_pieces_get() == n
        with ops.gru_step_pieces(2):
            assert lib.aslp_gru_step_pieces_get() == 2
            with ops.gru_step_pieces(1):
                assert lib.aslp_gru_step_pieces_get() == 1
            assert lib.aslp_gru_step_pieces_get() == 2
        assert lib.aslp_gru_step_pieces_get() == 0
        with pytest.raises(ZeroDivisionError):
            with ops.gru_step_pieces(1):
                1 / 0
        assert lib.aslp_gru_step_pieces_get() == 0         # restored although the body raised
        ops.set_gru_step_pieces(2)
        ops.set_gru_step_pieces(7)                          # anything else: back to the (unset) environment
        assert lib.aslp_gru_step_pieces_get() == 0
        seq = lib.aslp_gru_seq_pieces_get()
        with ops.gru_step_pieces(1):                        # the persistent GRU kernels' switch is another one
            assert lib.aslp_gru_seq_pieces_get() == seq
    finally:
        ops.set_gru_step_pieces(-1)
