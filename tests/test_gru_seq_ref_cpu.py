"""CPU-only: what tests/test_gru_seq_kernels_gpu.py stands on.
  * the float64 model of the aslp_gru_seq contract (tests/gru_seq_ref.py) is pinned to the oracle (orc_gru_forward / orc_gru_backward) at the
    oracle's own fp32 distance, on every case of the list;
  * the one-piece model (operands of the four recurrent products rounded to 11 significant bits) differs from the float64 model in every case,
    and its distance d_model stays below lstm_seq_ref.BAR_ONE_PIECE (2e-3 relative l2, 2e-2 element) per tensor: the weight range of
    build_case (W_SCALE = 0.08) was chosen here so that it does.  Worst d_model over all cases and tensors: relative l2 4.03e-4 (d_r of
    H512-S8-T3), element 6.30e-4 (m of H512-S8-T3) -- WORST_D_MODEL below;
  * the case list, taken over the piece counts, launches every one of the 12 persistent GRU kernels (two rungs x two passes x pieces 0 / 2 / 1),
    counted from the dispatch ladder restated here;
  * the binding declares the switch's three entry points."""
import ctypes

import numpy as np
import pytest

import gru_seq_ref as ref
import lstm_seq_ref

IDS = [ref.case_id(c) for c in ref.CASES]
WORST_D_MODEL = (4.03e-4, 6.30e-4)   # relative l2, element: as printed by test_one_piece_model_differs_and_stays_below_the_bar
_cache = {}


def case(k):
    if k not in _cache:
        inp = ref.build_case(ref.CASES[k])
        _cache[k] = (inp, ref.reference(inp))
    return _cache[k]


@pytest.mark.parametrize("k", range(len(ref.CASES)), ids=IDS)
def test_model_matches_oracle(oracle, k):
    """The oracle's fp32 buffers against the float64 model, the x-parts formed in float64 from the oracle's own input product: every activation
    and diff tensor within the bar the LSTM model's CPU test uses for the same comparison (lstm_seq_ref.BAR, 10 x that per element)."""
    c = ref.CASES[k]
    D, H, S, T = 7, c.H, c.S, c.T
    rng = np.random.default_rng([11, k])
    p = oracle.Gru(D, H, rng, scale=0.12)
    x = rng.standard_normal((T * S, D)).astype(np.float32)
    od = rng.standard_normal((T * S, H)).astype(np.float32)
    state = np.zeros((S, 5 * H), np.float32)
    if c.h0:
        state[:, 4 * H:] = rng.standard_normal((S, H)).astype(np.float32) * 0.5
    buf = p.forward(x, T, S, init_state=state)
    dbuf, _ = p.backward(od, T, S, buf)
    f64 = lambda a: np.asarray(a, np.float64)
    y = np.zeros((T + 2, S, 5 * H))
    y[1:T + 1, :, :3 * H] = (f64(x) @ f64(p.w_zrm_x).T + f64(p.bias)).reshape(T, S, 3 * H)
    y[0] = state
    d = np.zeros((T + 2, S, 5 * H))
    d[1:T + 1, :, 4 * H:] = f64(od).reshape(T, S, H)
    inp = dict(case=c, y=y, d=d, w_zr=p.w_zr_h, w_m=p.w_m_g)
    ry, rd = ref.reference(inp)
    dist = ref.distances(c, buf.reshape(T + 2, S, -1), dbuf.reshape(T + 2, S, -1), ry, rd)
    for name, (l2, el) in dist.items():
        assert l2 < lstm_seq_ref.BAR and el < 10 * lstm_seq_ref.BAR, (IDS[k], name, l2, el)
    assert set(dist) == {"z", "r", "m", "g", "h", "d_z", "d_r", "d_m", "d_g", "d_h"}


def test_one_piece_model_differs_and_stays_below_the_bar():
    assert ref.BAR == lstm_seq_ref.BAR == 1e-5 and ref.BAR_ONE_PIECE == lstm_seq_ref.BAR_ONE_PIECE == 2e-3
    worst = [0.0, 0.0, "", ""]
    for k, c in enumerate(ref.CASES):
        inp, (ry, rd) = case(k)
        y1, d1 = ref.reference_one_piece(inp)
        assert not np.array_equal(y1[1:], ry[1:]) and not np.array_equal(d1[1:c.T + 1], rd[1:c.T + 1]), (IDS[k], "a recurrent product ran in both passes")
        dm = ref.d_model(inp, (ry, rd))
        for name, (l2, el) in dm.items():
            assert l2 < ref.BAR_ONE_PIECE and el < 10 * ref.BAR_ONE_PIECE, (IDS[k], name, l2, el)   # (0 where no product precedes: d_h at T = 1)
            if l2 > worst[0]:
                worst[0], worst[2] = l2, "%s of %s" % (name, IDS[k])
            if el > worst[1]:
                worst[1], worst[3] = el, "%s of %s" % (name, IDS[k])
    print("gru-seq d_model worst: relative l2 %.2e (%s), element %.2e (%s)" % (worst[0], worst[2], worst[1], worst[3]))
    assert worst[0] <= 1.05 * WORST_D_MODEL[0] and worst[1] <= 1.05 * WORST_D_MODEL[1], "the docstring's figures are stale"


def test_round11_is_fp16s_significand():
    rng = np.random.default_rng(5)
    x = rng.standard_normal(4096) * 3.0            # inside fp16's normal range: the model's rounding is numpy's float16 rounding there
    assert np.array_equal(ref.round11(x), x.astype(np.float16).astype(np.float64))
    assert np.array_equal(ref.round11(x * 2.0 ** -40), ref.round11(x) * 2.0 ** -40) and np.array_equal(ref.round11(x * 2.0 ** 30), ref.round11(x) * 2.0 ** 30)
    assert ref.round11(0.0) == 0.0


# ---- the case list covers every instantiation --------------------------------------------------------------------------------------------

def launched(c, pieces):
    """(family, rung, pieces template parameter NP) of the forward and the backward launch of a case: pick_gru restated"""
    rung = 0 if c.H <= 128 else 1
    assert c.H <= 512 and pieces in (0, 1, 2)
    return [("gru_seq_fwd", rung, pieces), ("gru_seq_bwd", rung, pieces)]


def test_cases_reach_all_12_kernels():
    every = {(f, rung, p) for f in ("gru_seq_fwd", "gru_seq_bwd") for rung in (0, 1) for p in (0, 1, 2)}
    assert len(every) == 12 and ref.PIECES == (0, 2, 1)
    hit = {}
    for c in ref.CASES:
        for pieces in ref.PIECES:
            for inst in launched(c, pieces):
                hit.setdefault(inst, []).append(c)
    assert set(hit) == every, sorted(every - set(hit), key=str)
    for inst, cases in sorted(hit.items(), key=str):
        print("  %-11s rung %d pieces %d <- H = %s" % (inst + (sorted({c.H for c in cases}),)))


def test_case_list_holds_what_the_issue_names():
    cs = ref.CASES
    assert {c.H for c in cs} == {4, 20, 128, 132, 512} and {1, 8, 9, 64} <= {c.S for c in cs} and {1, 2, 5} <= {c.T for c in cs}
    assert all(c.T <= 6 for c in cs) and any(c.H == 512 and c.T == 3 for c in cs) and any(c.h0 for c in cs)
    assert any(c.S == 20 and (8, 12) in c.windows and len(c.windows) == 2 for c in cs)
    assert any((c.H, c.S, c.T) == (132, 9, 3) and not c.windows for c in cs)   # the magnitude test's case
    for c in cs:
        assert c.H % 4 == 0
        for s_begin, s_count in c.windows:
            assert s_begin + s_count <= c.S and (s_count + 7) // 8 <= 8
        inp = ref.build_case(c)
        assert inp["ld"] == 5 * c.H + 8 and inp["w_zr"].shape == (2 * c.H, c.H + 4) and inp["w_zr_t"].shape == (c.H, 2 * c.H + 4)
        assert inp["w_m"].shape == inp["w_m_t"].shape == (c.H, c.H + 4) and np.array_equal(inp["w_zr_t"][:, :2 * c.H], inp["w_zr"][:, :c.H].T)
        assert bool(inp["y"][0, :, 4 * c.H:5 * c.H].any()) == bool(c.h0)


def test_inputs_are_benign():
    """no saturated gates: a GPU comparison that fails cannot be blamed on the cases"""
    for k, c in enumerate(ref.CASES):
        _, (ry, _) = case(k)
        gates = np.abs(ry[1:c.T + 1, :, :3 * c.H])
        assert np.mean(gates > 0.999) < 0.01, IDS[k]


# ---- the binding ------------------------------------------------------------------------------------------------------------------------------

def test_binding_declares_the_switch(aslp):
    for name in ("aslp_gru_seq_pieces", "aslp_gru_seq_pieces_get", "aslp_gru_seq_last_pieces"):
        assert hasattr(aslp.lib, name), name
    assert list(aslp.lib.aslp_gru_seq_pieces.argtypes) == [ctypes.c_int] and aslp.lib.aslp_gru_seq_pieces.restype is None
    assert list(aslp.lib.aslp_gru_seq_pieces_get.argtypes) == [] and aslp.lib.aslp_gru_seq_pieces_get.restype is ctypes.c_int
    assert list(aslp.lib.aslp_gru_seq_last_pieces.argtypes) == [] and aslp.lib.aslp_gru_seq_last_pieces.restype is ctypes.c_int
    assert aslp.lib.aslp_gru_seq_last_pieces() in (0, 1, 2)


def test_switch_is_a_setting_of_its_own(aslp):
    lib, ops = aslp.lib, aslp.ops
    start = lib.aslp_gru_seq_pieces_get()
    lstm = (lib.aslp_lstm_operand_pieces_get(), lib.aslp_lstm_step_split16_get(), lib.aslp_gemm_operand_planes_get())
    try:
        for n in (0, 1, 2):
            ops.set_gru_seq_pieces(n)
            assert lib.aslp_gru_seq_pieces_get() == n
            assert (lib.aslp_lstm_operand_pieces_get(), lib.aslp_lstm_step_split16_get(), lib.aslp_gemm_operand_planes_get()) == lstm
        with ops.gru_seq_pieces(1):
            assert lib.aslp_gru_seq_pieces_get() == 1
            with ops.gru_seq_pieces(0):
                assert lib.aslp_gru_seq_pieces_get() == 0
            assert lib.aslp_gru_seq_pieces_get() == 1
        assert lib.aslp_gru_seq_pieces_get() == 2
        with pytest.raises(RuntimeError):
            with ops.gru_seq_pieces(1):
                raise RuntimeError("body")
        assert lib.aslp_gru_seq_pieces_get() == 2                  # restored although the body raised
        for other in (-1, 3, 7):                                   # anything else: back to the environment
            ops.set_gru_seq_pieces(2 if start != 2 else 1)
            ops.set_gru_seq_pieces(other)
            assert lib.aslp_gru_seq_pieces_get() == start, other
        with ops.lstm_operand_pieces(1):                           # and the LSTM switch does not reach it
            assert lib.aslp_gru_seq_pieces_get() == start
    finally:
        ops.set_gru_seq_pieces(-1)
    assert lib.aslp_gru_seq_pieces_get() == start
