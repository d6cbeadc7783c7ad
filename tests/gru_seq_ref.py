"""A plain numpy model of the aslp_gru_seq contract (include/aslp_kernels.h: aslp_gru_seq) in the arithmetic order of
oracle/aslp_oracle_rnn.c (orc_gru_forward / orc_gru_backward) -- written from those two texts, not from the kernels -- and what the tests
around it share: the case list, one seeded case builder and the ctypes driver of aslp_gru_seq_forward / _backward.

    forward(inp)                 activations [(T+2), S, 5H], float64
    backward(inp, y)             diffs of the same shape
    reference(inp)               both
    reference_one_piece(inp)     the same recurrence with the operands of the four recurrent products (left operand and weights) rounded to
                                 fp16's 11 significant bits and nothing else changed: what aslp_gru_seq_pieces(1) computes, up to fp32 rounding.
                                 The kernels' power-of-two scales do not change that rounding, so no scale appears here.

Buffers: rows (T+2) S, row = t S + s; columns [z|r|m|g|h], H each.  Row block 0 of y holds the carried history h(0); the recursion runs
t = 1..T, BPTT t = T..1 from the zero row block T+1."""
import collections
import ctypes as C

import numpy as np

import lstm_seq_ref

BAR = lstm_seq_ref.BAR                       # relative l2 error per tensor against float64 (10 x that per element): pieces 0 and 2
BAR_ONE_PIECE = lstm_seq_ref.BAR_ONE_PIECE   # the model's own one-piece distance stays below this (and 10 x per element)
CANARY = -7.25                               # pad columns no launch may touch
PIECES = (0, 2, 1)                           # every case runs under these, in this order
NAMES = ("z", "r", "m", "g", "h")

Case = collections.namedtuple("Case", "H S T h0 windows")
# h0: the carried history is non-zero; windows: () = one launch for all S streams, else the (s_begin, s_count) launches of a pass
CASES = [
    Case(4, 1, 1, 1, ()),                    # one workgroup holding 4 of 16 cells, waves 1..7 with empty K slices; T = 1: the backward kernel's first product never runs
    Case(20, 9, 2, 0, ()),                   # second workgroup of 4 cells; second chain of one stream; zero history
    Case(128, 64, 2, 1, ()),                 # top of the lower rung, all 8 chains
    Case(132, 9, 5, 1, ()),                  # first of the upper rung: K slices of 24 (forward) and 40 (backward), no multiples of 32; wave 5 half, waves 6, 7 beyond K
    Case(132, 9, 3, 1, ()),                  # (the case of the magnitude test)
    Case(132, 20, 2, 1, ((0, 8), (8, 12))),  # stream windows: two launches per pass, the second s_begin = 8, s_count = 12
    Case(512, 8, 3, 1, ()),                  # the full grid of 8 x 32 workgroups, every K slice whole
]


def case_id(c):
    return "H%d-S%d-T%d%s%s" % (c.H, c.S, c.T, "" if c.h0 else "-h0zero", "-win" if c.windows else "")


def launches(c):
    return c.windows if c.windows else ((0, 0),)


W_SCALE = 0.08   # standard deviation of the recurrent weights (chosen in tests/test_gru_seq_ref_cpu.py: the model's one-piece distance stays below BAR_ONE_PIECE)


def build_case(c):
    """Seeded inputs of a case, float32, in the padded layout the launches get: ld = 5H + 8, ldw = K + 4 (forward W_zr_h [2H x H] and W_m_g
    [H x H]; backward their transposes [H x 2H], [H x H]), every pad column holding CANARY.  Scales: gate pre-activations and dL/dh 1,
    history 0.5, weights W_SCALE."""
    H, S, T = c.H, c.S, c.T
    rng = np.random.default_rng([c.H, c.S, c.T, c.h0, len(c.windows)])
    rnd = lambda *shape, scale=1.0: (rng.standard_normal(shape) * scale).astype(np.float32)
    ld = 5 * H + 8
    y = np.zeros((T + 2, S, ld), np.float32)
    y[1:T + 1, :, :3 * H] = rnd(T, S, 3 * H)               # x-parts + bias of z, r, m
    if c.h0:
        y[0, :, 4 * H:5 * H] = rnd(S, H, scale=0.5)        # h(0)
    y[:, :, 5 * H:] = CANARY
    d = np.zeros((T + 2, S, ld), np.float32)
    d[1:T + 1, :, 4 * H:5 * H] = rnd(T, S, H)              # the loss's share of d_h
    d[:, :, 5 * H:] = CANARY

    def padded(m):
        out = np.full((m.shape[0], m.shape[1] + 4), CANARY, np.float32)
        out[:, :m.shape[1]] = m
        return out
    w_zr, w_m = rnd(2 * H, H, scale=W_SCALE), rnd(H, H, scale=W_SCALE)
    return dict(case=c, ld=ld, y=y, d=d, w_zr=padded(w_zr), w_m=padded(w_m), w_zr_t=padded(w_zr.T), w_m_t=padded(w_m.T))


# ---- the model ----------------------------------------------------------------------------------------------------------------------

def _sigm(x):
    e = np.exp(-np.abs(x))
    return np.where(x > 0, 1 / (1 + e), e / (1 + e))


def round11(x):
    """x rounded to 11 significant bits, nearest even (fp16's significand without its exponent range)"""
    m, e = np.frexp(np.asarray(x, np.float64))
    return np.ldexp(np.round(m * 2048.0) / 2048.0, e)


def forward(inp, rnd=None):
    c = inp["case"]
    H, T = c.H, c.T
    q = rnd if rnd is not None else (lambda a: a)
    oz, orr, om, og, oh = (k * H for k in range(5))
    sl = lambda o: slice(o, o + H)
    y = inp["y"][:, :, :5 * H].astype(np.float64)
    y[1:T + 1, :, og:] = 0.0
    w_zr, w_m = q(inp["w_zr"][:, :H].astype(np.float64)), q(inp["w_m"][:, :H].astype(np.float64))
    for t in range(1, T + 1):
        hp = y[t - 1, :, sl(oh)]
        zr = _sigm(y[t, :, :2 * H] + q(hp) @ w_zr.T)
        z, r = zr[:, :H], zr[:, H:]
        g = r * hp
        m = np.tanh(y[t, :, sl(om)] + q(g) @ w_m.T)
        h = hp - hp * z + z * m
        y[t, :, sl(oz)], y[t, :, sl(orr)], y[t, :, sl(om)], y[t, :, sl(og)], y[t, :, sl(oh)] = z, r, m, g, h
    return y


def backward(inp, y, rnd=None):
    c = inp["case"]
    H, T = c.H, c.T
    q = rnd if rnd is not None else (lambda a: a)
    oz, orr, om, og, oh = (k * H for k in range(5))
    sl = lambda o: slice(o, o + H)
    d = inp["d"][:, :, :5 * H].astype(np.float64)
    w_zr, w_m = q(inp["w_zr"][:, :H].astype(np.float64)), q(inp["w_m"][:, :H].astype(np.float64))
    dsigm = lambda yy, e: e * yy * (1 - yy)
    dtanh = lambda yy, e: e * (1 - yy * yy)
    for t in range(T, 0, -1):
        dn, yn, yt, hp = d[t + 1], y[t + 1], y[t], y[t - 1, :, sl(oh)]
        dh = d[t, :, sl(oh)] + q(dn[:, :2 * H]) @ w_zr
        dh = dh + dn[:, sl(oh)] - dn[:, sl(oh)] * yn[:, sl(oz)] + dn[:, sl(og)] * yn[:, sl(orr)]
        dm = dtanh(yt[:, sl(om)], dh * yt[:, sl(oz)])
        dg = q(dm) @ w_m
        dr = dsigm(yt[:, sl(orr)], dg * hp)
        dz = dsigm(yt[:, sl(oz)], dh * yt[:, sl(om)] - dh * hp)
        d[t, :, sl(oz)], d[t, :, sl(orr)], d[t, :, sl(om)], d[t, :, sl(og)], d[t, :, sl(oh)] = dz, dr, dm, dg, dh
    return d


def reference(inp):
    """(y, d) of the model, float64"""
    y = forward(inp)
    return y, backward(inp, y)


def reference_one_piece(inp):
    y = forward(inp, round11)
    return y, backward(inp, y, round11)


def tensors(c, backward_pass):
    """(name, column offset) of what a pass leaves and the tests compare, H columns each"""
    return [(("d_" if backward_pass else "") + n, k * c.H) for k, n in enumerate(NAMES)]


# ---- the launches ----------------------------------------------------------------------------------------------------------------------

def gru_args(aslp, inp, y, d, w_zr, w_m, backward_pass):
    c = inp["case"]
    a = aslp._lib.GruSeq()
    a.y, a.d, a.w_zr, a.w_m = y.data_ptr(), (d.data_ptr() if d is not None else None), w_zr.data_ptr(), w_m.data_ptr()
    a.ldw_zr, a.ldw_m = (2 * c.H + 4 if backward_pass else c.H + 4), c.H + 4
    a.ld, a.T, a.S, a.H = inp["ld"], c.T, c.S, c.H
    return a


def run_on_gpu(aslp, torch, dev, inp, pieces, want_pieces, d_scale=1.0):
    """Both passes of a case on the GPU under aslp_gru_seq_pieces(pieces), through the C ABI: aslp_lstm_seq_fill, the x-parts and the history,
    aslp_gru_seq_forward, then aslp_gru_seq_backward on what it left -- one launch per stream window.  After every launch: the error state,
    aslp_gru_seq_last_pieces() == want_pieces, and bit for bit everything the launch has no business writing (pad columns, streams outside the
    window, row blocks 0 and T+1, the weights, y during the backward pass).  d_scale multiplies the loss's share of d_h.  Returns numpy copies
    of the y and d columns [0, 5H)."""
    lib, c = aslp.lib, inp["case"]
    H, S, T, ld = c.H, c.S, c.T, inp["ld"]
    same = lambda a, b: np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    y = torch.zeros((T + 2) * S, ld, device=dev)
    lib.aslp_lstm_seq_fill(y.data_ptr(), ld, T, S, 3 * H, 2 * H)           # g and h start as "not yet published"; before anything is stored
    yv, y0 = y.view(T + 2, S, ld), to_dev(inp["y"])
    yv[1:T + 1, :, :3 * H] = y0[1:T + 1, :, :3 * H]
    yv[0] = y0[0]
    yv[:, :, 5 * H:] = CANARY
    d = torch.zeros((T + 2) * S, ld, device=dev)
    lib.aslp_lstm_seq_fill(d.data_ptr(), ld, T, S, 0, 3 * H)
    dv = d.view(T + 2, S, ld)
    dv[1:T + 1, :, 4 * H:5 * H] = to_dev((inp["d"][1:T + 1, :, 4 * H:5 * H].astype(np.float64) * d_scale).astype(np.float32))
    dv[:, :, 5 * H:] = CANARY
    w = {k: to_dev(inp[k]) for k in ("w_zr", "w_m", "w_zr_t", "w_m_t")}
    readonly = lambda: [w[k].cpu().numpy() for k in sorted(w)]
    ro0 = readonly()
    bufs = dict(y=y, d=d)
    out = {}
    lib.aslp_gru_seq_pieces(pieces)
    try:
        for backward_pass, buf in ((0, "y"), (1, "d")):
            a = gru_args(aslp, inp, y, d if backward_pass else None, w["w_zr_t" if backward_pass else "w_zr"], w["w_m_t" if backward_pass else "w_m"], backward_pass)
            y_before_bwd = y.cpu().numpy()
            for s_begin, s_count in launches(c):
                a.s_begin, a.s_count = s_begin, s_count
                before = bufs[buf].cpu().numpy().reshape(T + 2, S, ld)
                assert lib.aslp_gru_seq_supported(C.byref(a), backward_pass) == 1, (case_id(c), "pieces", pieces, backward_pass, s_begin, s_count)
                (lib.aslp_gru_seq_backward if backward_pass else lib.aslp_gru_seq_forward)(C.byref(a))
                torch.cuda.synchronize()
                aslp._lib.check_error()
                assert lib.aslp_gru_seq_last_pieces() == want_pieces, (case_id(c), lib.aslp_gru_seq_last_pieces(), want_pieces)
                after = bufs[buf].cpu().numpy().reshape(T + 2, S, ld)
                lo, hi = (s_begin, s_begin + s_count) if s_count else (0, S)
                what = (case_id(c), "pieces", pieces, buf, "window", s_begin, s_count)
                assert same(before[:, :, 5 * H:], after[:, :, 5 * H:]), what + ("pad columns",)
                assert same(before[:, :lo], after[:, :lo]) and same(before[:, hi:], after[:, hi:]), what + ("streams outside the window",)
                assert same(before[[0, T + 1]], after[[0, T + 1]]), what + ("row blocks 0 and T+1",)
                for r0, r1 in zip(ro0, readonly()):
                    assert same(r0, r1), what + ("a weight matrix",)
                if backward_pass:
                    assert same(y_before_bwd, y.cpu().numpy()), what + ("the backward pass wrote into y",)
            out[buf] = bufs[buf].cpu().numpy().reshape(T + 2, S, ld)[:, :, :5 * H].copy()
    finally:
        lib.aslp_gru_seq_pieces(-1)
    return out


errors = lstm_seq_ref.errors   # (relative l2 error, largest element error relative to max(1, largest |reference|)) of one tensor


def distances(c, y, d, ref_y, ref_d):
    """{tensor name: (relative l2, element)} of a run (y, d) against a reference, row blocks 1..T"""
    out = {}
    for backward_pass, g, r in ((0, y, ref_y), (1, d, ref_d)):
        for name, off in tensors(c, backward_pass):
            a = g[1:c.T + 1, :, off:off + c.H]
            out[name] = errors(a, r[1:c.T + 1, :, off:off + c.H]) if np.isfinite(a).all() else (np.inf, np.inf)
    return out


def compare(inp, got, ref_y, ref_d, bars):
    """Every tensor of both passes against the model; bars: one (l2, element) pair for all tensors, or {name: pair}.  Returns the distances
    after asserting each below its bar."""
    c = inp["case"]
    dist = distances(c, got["y"], got["d"], ref_y, ref_d)
    fails = []
    for name, (l2, el) in dist.items():
        b_l2, b_el = bars[name] if isinstance(bars, dict) else bars
        if not (l2 < b_l2 and el < b_el):
            fails.append((case_id(c), name, l2, el, "bar", b_l2, b_el))
    assert not fails, fails
    return dist


def d_model(inp, ref=None):
    """{tensor name: (relative l2, element)}: the distance of the one-piece model from the float64 model"""
    ref_y, ref_d = ref if ref is not None else reference(inp)
    y1, d1 = reference_one_piece(inp)
    return distances(inp["case"], y1, d1, ref_y, ref_d)
