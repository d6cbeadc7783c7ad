"""A float64 numpy model of ONE timestep of the step-fused LSTM path (include/aslp_kernels.h aslp_lstm_step_forward / _backward and their
split-fp16 counterparts aslp_lstm_step_forward_h / _backward_h; csrc/rnn_fused.hip), for one direction.  No GPU, no library.

Row blocks are [S, width] arrays with the engine's column order g | i | f | o | c | h | m (no i with coupled gates).  `pieces` rounds the
OPERANDS of the two products as the numeric contract of aslp_lstm_step_split16 says and leaves everything else in float64:
  0   unrounded;
  2   22 bits behind the scale: x s = hi + 2^-11 lo', hi = fp16(x s), lo' = fp16((x s - hi) 2^11);
  1   fp16 behind the scale: hi alone.
The scales are powers of two that put the largest |value| they cover into [2^13, 2^14) (csrc/split16.h s16_exponent; nothing to cover: 1):
the weights' covers the whole matrix, m(t-1) has none (|m| <= 1), dGATES(next) has one per stream row and run of 128 consecutive k, runs
counted from the start of each of the 32 K parts (8 workgroups x 4 waves) the backward product is split into."""
import numpy as np

K_PARTS = 32      # kKQ x kNW of csrc/rnn_fused.hip
RUN_STEPS = 8     # 16-wide k steps per run (kRunH)


def gates(cifg):
    return 3 if cifg else 4


def cols(C, cifg):
    """og, oi, of, oo, oc, oh, om"""
    return (0, None, C, 2 * C, 3 * C, 4 * C, 5 * C) if cifg else (0, C, 2 * C, 3 * C, 4 * C, 5 * C, 6 * C)


def sigm(x):
    e = np.exp(-np.abs(x))
    return np.where(x > 0, 1 / (1 + e), e / (1 + e))


def pow2_scale(bound):
    """the scale of csrc/split16.h for a bound (array or scalar): 2^(14 - e) with bound = f 2^e, f in [0.5, 1); 1 for a zero bound"""
    b = np.asarray(bound, np.float64)
    _, e = np.frexp(np.where(b > 0, b, 1.0))
    return np.where(b > 0, np.ldexp(1.0, np.clip(14 - e, -120, 120)), 1.0)


def round_pieces(x, pieces, scale=1.0):
    """x as the product sees it with `pieces` fp16 pieces behind `scale` (broadcast against x)"""
    x = np.asarray(x, np.float64)
    if pieces == 0:
        return x
    y = x * scale
    with np.errstate(over="ignore"):
        hi = y.astype(np.float16).astype(np.float64)
        if pieces == 1:
            return hi / scale
        lo = ((y - hi) * 2048.0).astype(np.float16).astype(np.float64)
    return (hi + lo / 2048.0) / scale


def weight_operand(w, pieces):
    w = np.asarray(w, np.float64)
    return round_pieces(w, pieces, pow2_scale(np.abs(w).max() if w.size else 0.0))


def dgates_runs(K):
    """[(k0, k1)]: the runs of consecutive k one scale covers, over the backward product's K = G C"""
    nst = (K + 15) // 16
    per = (nst + K_PARTS - 1) // K_PARTS
    runs = []
    for part in range(K_PARTS):
        qend = min(nst, (part + 1) * per)
        for q0 in range(part * per, qend, RUN_STEPS):
            runs.append((16 * q0, min(16 * min(q0 + RUN_STEPS, qend), K)))
    return runs


def dgates_operand(dg, pieces):
    dg = np.asarray(dg, np.float64)
    if pieces == 0:
        return dg
    out = np.empty_like(dg)
    runs = dgates_runs(dg.shape[1])
    assert runs[0][0] == 0 and runs[-1][1] == dg.shape[1] and all(a[1] == b[0] for a, b in zip(runs, runs[1:]))
    for k0, k1 in runs:
        blk = dg[:, k0:k1]
        out[:, k0:k1] = round_pieces(blk, pieces, pow2_scale(np.abs(blk).max(axis=1, keepdims=True)))
    return out


def forward(y_cur, y_prev, w_eff, peep_i, peep_f, peep_o, cifg, masked=None, no_product=False, pieces=0):
    """y_cur [S, >= (G + 3) C]: gate columns hold the x-part + bias; returns the row block after the step (float64).
    w_eff [G C, C]; masked: bool [S] (streams whose sequence has ended: every column of the step is zero)."""
    C = w_eff.shape[1]
    G = gates(cifg)
    og, oi, of, oo, oc, oh, om = cols(C, cifg)
    sl = lambda o: slice(o, o + C)
    f64 = lambda a: np.asarray(a, np.float64)
    y = f64(y_cur).copy()
    yp = f64(y_prev)
    pre = y[:, :G * C].copy()
    if not no_product:
        pre += round_pieces(yp[:, sl(om)], pieces) @ weight_operand(w_eff, pieces).T
    cp = yp[:, sl(oc)]
    g = np.tanh(pre[:, sl(og)])
    f = sigm(pre[:, sl(of)] + cp * f64(peep_f))
    if cifg:
        cc = -g * f + g + cp * f
    else:
        i = sigm(pre[:, sl(oi)] + cp * f64(peep_i))
        cc = g * i + cp * f
        y[:, sl(oi)] = i
    cc = np.clip(cc, -50, 50)
    h = np.tanh(cc)
    o = sigm(pre[:, sl(oo)] + cc * f64(peep_o))
    y[:, sl(og)], y[:, sl(of)], y[:, sl(oo)] = g, f, o
    y[:, sl(oc)], y[:, sl(oh)], y[:, sl(om)] = cc, h, h * o
    if masked is not None:
        y[np.asarray(masked, bool), :(G + 3) * C] = 0
    return y


def backward_product(d_next, w_eff_t, cifg, pieces=0):
    """dGATES(next) W_eff [S, C] as the backward step forms it; w_eff_t [C, G C]"""
    C = w_eff_t.shape[0]
    G = gates(cifg)
    return dgates_operand(np.asarray(d_next, np.float64)[:, :G * C], pieces) @ weight_operand(w_eff_t, pieces).T


def backward(d_cur, d_next, y_cur, y_next, y_prev, w_eff_t, peep_i, peep_f, peep_o, cifg, has_next=True, pieces=0):
    """d_cur [S, >= (G + 3) C]: the m columns hold dL/dm from above; returns the diff row block after the step (float64).  With has_next
    false the product is not formed and the m columns stay as they came.  No masking of its own: the zeroed rows of y carry it."""
    C = w_eff_t.shape[0]
    G = gates(cifg)
    og, oi, of, oo, oc, oh, om = cols(C, cifg)
    sl = lambda o: slice(o, o + C)
    f64 = lambda a: np.asarray(a, np.float64)
    d, dn, y, yn, yp = f64(d_cur).copy(), f64(d_next), f64(y_cur), f64(y_next), f64(y_prev)
    dsigm = lambda yy, e: e * yy * (1 - yy)
    dtanh = lambda yy, e: e * (1 - yy * yy)
    dm = d[:, sl(om)]
    if has_next:
        dm = dm + backward_product(dn, w_eff_t, cifg, pieces)
        d[:, sl(om)] = dm
    yo, yh, yg, yf = y[:, sl(oo)], y[:, sl(oh)], y[:, sl(og)], y[:, sl(of)]
    dh = dtanh(yh, dm * yo)
    do = dsigm(yo, dm * yh)
    dc = dh + dn[:, sl(oc)] * yn[:, sl(of)]
    if not cifg:
        dc = dc + dn[:, sl(oi)] * f64(peep_i)
    dc = dc + dn[:, sl(of)] * f64(peep_f)
    dc = dc + do * f64(peep_o)
    cp = yp[:, sl(oc)]
    d[:, sl(oh)], d[:, sl(oo)], d[:, sl(oc)] = dh, do, dc
    if cifg:
        d[:, sl(of)] = dsigm(yf, dc * cp - dc * yg)
        d[:, sl(og)] = dtanh(yg, dc - dc * yf)
    else:
        yi = y[:, sl(oi)]
        d[:, sl(of)] = dsigm(yf, dc * cp)
        d[:, sl(oi)] = dsigm(yi, dc * yg)
        d[:, sl(og)] = dtanh(yg, dc * yi)
    return d


def errors(got, ref):
    """(relative l2, largest element error relative to max(1, largest |ref|)) -- the two figures of tests/lstm_seq_ref.py"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    den = np.linalg.norm(ref)
    l2 = float(np.linalg.norm(got - ref) / den) if den > 0 else float(np.linalg.norm(got - ref))
    el = float(np.max(np.abs(got - ref)) / max(1.0, float(np.max(np.abs(ref))))) if ref.size else 0.0
    return l2, el
