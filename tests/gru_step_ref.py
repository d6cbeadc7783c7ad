"""A float64 numpy model of ONE timestep of the step-fused GRU path (include/aslp_kernels.h aslp_gru_step_forward / _backward and their
fp16-piece counterparts aslp_gru_step_forward_h / _backward_h; csrc/gru_fused.hip), and the inputs the direct GPU cases share with the CPU
test that bounds the model's own rounding distance.  No GPU, no library.

Row blocks are [S, width] arrays with the engine's column order z | r | m | g | h, H each.  `pieces` rounds the OPERANDS of the four
products as the numeric contract of aslp_gru_step_pieces says and leaves everything else in float64:
  0   unrounded;
  2   22 bits behind the scale: x s = hi + 2^-11 lo', hi = fp16(x s), lo' = fp16((x s - hi) 2^11);
  1   fp16 behind the scale: hi alone.
The scales are powers of two that put the largest |value| they cover into [2^13, 2^14) (csrc/split16.h s16_exponent; nothing to cover: 1):
a weight matrix has one, h(t-1) and g(t) have none (both bounded by 1), [d_z | d_r](t+1) and d_m(t) have one per stream row and run of 128
consecutive k, runs counted from the start of each of the 4 waves' K slices (contiguous, in 16-wide k steps)."""
import numpy as np

from lstm_step_ref import errors, pow2_scale, round_pieces, sigm, weight_operand   # the split itself is the LSTM step path's

WAVES = 4         # K slices of every product (kBwd1Waves is 4 too)
RUN_STEPS = 8     # 16-wide k steps per run (kRunH)
NAMES = ("z", "r", "m", "g", "h")


def diff_runs(K):
    """[(k0, k1)]: the runs of consecutive k one scale covers, over a backward product's K"""
    nst = (K + 15) // 16
    per = (nst + WAVES - 1) // WAVES
    runs = []
    for wave in range(WAVES):
        qend = min(nst, (wave + 1) * per)
        for q0 in range(wave * per, qend, RUN_STEPS):
            runs.append((16 * q0, min(16 * min(q0 + RUN_STEPS, qend), K)))
    return runs


def diff_operand(dx, pieces):
    dx = np.asarray(dx, np.float64)
    if pieces == 0:
        return dx
    out = np.empty_like(dx)
    runs = diff_runs(dx.shape[1])
    assert runs[0][0] == 0 and runs[-1][1] == dx.shape[1] and all(a[1] == b[0] for a, b in zip(runs, runs[1:]))
    for k0, k1 in runs:
        blk = dx[:, k0:k1]
        out[:, k0:k1] = round_pieces(blk, pieces, pow2_scale(np.abs(blk).max(axis=1, keepdims=True)))
    return out


def forward(y_cur, y_prev, w_zr_h, w_m_g, pieces=0):
    """y_cur [S, >= 5H]: columns z, r, m hold the x-part + bias; y_prev: the row block of t - 1; w_zr_h [2H, H], w_m_g [H, H].
    Returns the row block after the step (float64)."""
    H = w_m_g.shape[0]
    f64 = lambda a: np.asarray(a, np.float64)
    y, hp = f64(y_cur).copy(), f64(y_prev)[:, 4 * H:5 * H]
    zr = sigm(y[:, :2 * H] + round_pieces(hp, pieces) @ weight_operand(w_zr_h, pieces).T)
    z, r = zr[:, :H], zr[:, H:]
    g = r * hp
    m = np.tanh(y[:, 2 * H:3 * H] + round_pieces(g, pieces) @ weight_operand(w_m_g, pieces).T)
    h = hp - hp * z + z * m
    y[:, :5 * H] = np.concatenate([z, r, m, g, h], axis=1)
    return y


def backward(d_cur, d_next, y_cur, y_next, y_prev, w_zr_h_t, w_m_g_t, has_next=True, pieces=0):
    """d_cur [S, >= 5H]: the h columns hold the loss's share of d_h; w_zr_h_t [H, 2H], w_m_g_t [H, H] (the transposes, as the kernels read
    them).  has_next false: the first product is not formed (the other terms of d_h(t+1) still enter).  Returns the diff row block after
    the step (float64)."""
    H = w_m_g_t.shape[0]
    f64 = lambda a: np.asarray(a, np.float64)
    d, dn, y, yn, hp = f64(d_cur).copy(), f64(d_next), f64(y_cur), f64(y_next), f64(y_prev)[:, 4 * H:5 * H]
    sl = lambda k: slice(k * H, (k + 1) * H)
    dsigm = lambda yy, e: e * yy * (1 - yy)
    dtanh = lambda yy, e: e * (1 - yy * yy)
    dh = d[:, sl(4)]
    if has_next:
        dh = dh + diff_operand(dn[:, :2 * H], pieces) @ weight_operand(w_zr_h_t, pieces).T
    dh = dh + dn[:, sl(4)] - dn[:, sl(4)] * yn[:, sl(0)] + dn[:, sl(3)] * yn[:, sl(1)]
    dm = dtanh(y[:, sl(2)], dh * y[:, sl(0)])
    dg = diff_operand(dm, pieces) @ weight_operand(w_m_g_t, pieces).T
    dr = dsigm(y[:, sl(1)], dg * hp)
    dz = dsigm(y[:, sl(0)], dh * y[:, sl(2)] - dh * hp)
    d[:, :5 * H] = np.concatenate([dz, dr, dm, dg, dh], axis=1)
    return d


def recurrence(inp, pieces=0):
    """T steps of the model on a case of tests/gru_seq_ref.py (its y / d buffers [(T + 2), S, >= 5H], w_zr [2H, >= H], w_m [H, >= H]):
    (y, d) as gru_seq_ref.reference returns them"""
    c = inp["case"]
    H, T = c.H, c.T
    y = np.asarray(inp["y"], np.float64)[:, :, :5 * H].copy()
    y[1:T + 1, :, 3 * H:] = 0.0
    d = np.asarray(inp["d"], np.float64)[:, :, :5 * H].copy()
    w_zr, w_m = np.asarray(inp["w_zr"], np.float64)[:, :H], np.asarray(inp["w_m"], np.float64)[:, :H]
    for t in range(1, T + 1):
        y[t] = forward(y[t], y[t - 1], w_zr, w_m, pieces)
    for t in range(T, 0, -1):
        d[t] = backward(d[t], d[t + 1], y[t], y[t + 1], y[t - 1], w_zr.T, w_m.T, has_next=t < T, pieces=pieces)
    return y, d


# ---- the inputs of the direct GPU cases (tests/test_gru_step_pieces_gpu.py) --------------------------------------------------------------------

# H: 4 (K below one 16-wide step), 20 / 36 / 132 (k tails of 4; K = 2H for the first backward product; wave slices that end inside K; a
# last column block of 4 cells for the 16-cell kernel at 20 and 36, for the 32-cell kernels at 36 and 132);  S: 1, 31 (a partial stream
# block), 33 (a second block holding one stream)
SHAPES = [(H, S) for H in (4, 20, 36, 132) for S in (1, 31, 33)]


def step_inputs(H, S):
    """float32 host arrays of one step, [S, 5H] row blocks: activations uniform in their ranges, weights uniform +-0.5 / sqrt(H), the rows of
    the next step's diffs scaled by exp(U(ln 1e-3, ln 10)), one of them with an all-zero [d_z | d_r]"""
    rng = np.random.default_rng(200 + H + S)
    W = 5 * H

    def act():
        return np.concatenate([rng.uniform(0.05, 0.95, (S, 2 * H)), rng.uniform(-0.95, 0.95, (S, 3 * H))], axis=1)
    h = dict(y_prev=act(), y_next=act(), y_act=act())
    h["y_x"] = np.concatenate([rng.standard_normal((S, 3 * H)), np.zeros((S, 2 * H))], axis=1)   # forward: x-part + bias of z, r, m
    rows = np.exp(rng.uniform(np.log(1e-3), np.log(10.0), (S, 1)))
    h["d_next"] = rng.standard_normal((S, W)) * rows
    h["zero_row"] = S // 2
    h["d_next"][h["zero_row"], :2 * H] = 0.0
    h["d_cur"] = np.concatenate([np.zeros((S, 4 * H)), rng.standard_normal((S, H)) * rows], axis=1)   # the loss's share of d_h
    h["w_zr"] = rng.uniform(-1, 1, (2 * H, H)) * 0.5 / np.sqrt(H)
    h["w_m"] = rng.uniform(-1, 1, (H, H)) * 0.5 / np.sqrt(H)
    return {k: (v.astype(np.float32) if isinstance(v, np.ndarray) else v) for k, v in h.items()}


def step_model(h, pieces, has_next=True):
    """(forward row block, backward row block) of the model on step_inputs"""
    return (forward(h["y_x"], h["y_prev"], h["w_zr"], h["w_m"], pieces),
            backward(h["d_cur"], h["d_next"], h["y_act"], h["y_next"], h["y_prev"], h["w_zr"].T, h["w_m"].T, has_next=has_next, pieces=pieces))


def step_errors(got, want, H):
    """{tensor: (relative l2, element)} of a (forward, backward) pair of [S, >= 5H] row blocks against another"""
    out = {}
    for p, prefix in enumerate(("", "d_")):
        for k, name in enumerate(NAMES):
            out[prefix + name] = errors(got[p][:, k * H:(k + 1) * H], want[p][:, k * H:(k + 1) * H])
    return out
