"""A plain numpy model of the aslp_lstm_seq contract (include/aslp_kernels.h: aslp_lstm_seq, aslp_lstm_cell_forward / _backward, the
fused-step note) in the arithmetic order of oracle/aslp_oracle_rnn.c -- written from those two texts, not from the kernels -- and what the
tests around it share: the case list, one seeded case builder and the ctypes driver of aslp_lstm_seq_forward / _backward.

    forward(inp, d)              activations [(T+2), S, (G+3) C] of direction d, float64 (or float32: the "inputs are benign" check)
    backward(inp, d, y)          diffs of the same shape (gate columns, d_c, d_h; the m columns hold the accumulated d_m)
    grad_partial(inp, d, y, dd)  the seven per-chain sums of a launch over the stream window [s_begin, s_begin + s_count)
    dmax(inp, dd)                largest finite |dGATES| of a direction

Buffers: rows (T+2) S, row = t S + s; columns [g|i|f|o|c|h|m] ([g|f|o|c|h|m] with coupled gates), C each.  The recursion of direction 0
starts from row block 0 and runs t = 1..T; `reverse` starts from row block T+1 and runs t = T..1; BPTT runs against it."""
import collections
import ctypes as C

import numpy as np

BAR = 1e-5              # relative l2 error per tensor against float64 (10 x that per element): two-piece, fp32-instruction, exact-activation kernels
BAR_ONE_PIECE = 2e-3    # ... with one fp16 piece per operand (the bar of tests/test_lstm_one_piece_gpu.py)
CANARY = -7.25          # pad columns, rows and vectors no launch may touch
SWITCHES = (("default", -1, -1, 2), ("split16=0", 0, -1, 0), ("pieces=1", -1, 1, 1))   # label, aslp_lstm_split16, aslp_lstm_operand_pieces, last_pieces

Case = collections.namedtuple("Case", "C S T ndir cifg ragged k_first col_first skip gp dmax windows")
# windows: () = one launch for all S streams, else the (s_begin, s_count) launches of a pass, one after the other
CASES = [
    Case(4, 1, 1, 1, 0, 0, 0, 0, 0, 1, 1, ()),          # one workgroup holding 4 of 16 cells, K = 4 in wave 0 alone; T = 1: no hand-off
    Case(4, 5, 2, 2, 1, 1, 4, 4, 0, 1, 0, ()),          # ... with coupled gates, both directions, r(0) W_first^T at k_first = 4, col_first 4
    Case(20, 9, 6, 1, 0, 1, 0, 0, 1, 1, 1, ()),         # two workgroups, the last of 4 cells; one full chain and one stream; skip_first_product
    Case(20, 5, 9, 2, 1, 1, 0, 0, 0, 0, 1, ()),         # the backward ring of 4 wraps twice; grad_partial off
    Case(36, 9, 2, 2, 0, 0, 4, 0, 0, 1, 0, ()),         # kw = 8: wave 4 half beyond K
    Case(128, 32, 6, 2, 0, 1, 128, 0, 0, 1, 1, ()),     # top of the small rung, all 8 chains; the largest k_first the small rung stages
    Case(128, 64, 2, 1, 1, 0, 40, 8, 0, 1, 0, ()),      # 8 chains of one direction
    Case(132, 5, 6, 1, 1, 0, 256, 0, 0, 0, 1, ()),      # bottom of the large rung: 9 workgroups, the last of 4 cells, wave 7 empty; k_first 256
    Case(132, 9, 9, 2, 0, 1, 0, 0, 0, 1, 1, ()),
    Case(132, 33, 2, 2, 1, 1, 0, 0, 0, 1, 1, ((0, 32), (32, 1))),   # more streams than one bidirectional launch takes
    Case(256, 9, 2, 1, 1, 0, 0, 0, 1, 1, 0, ()),        # top of lstm_seq_fwd_h NCH = 1
    Case(260, 5, 6, 2, 0, 1, 40, 4, 0, 1, 1, ()),       # bottom of NCH = 2: 17 workgroups, the last partial
    Case(260, 20, 2, 1, 1, 0, 0, 0, 0, 1, 1, ((8, 5),)),            # a window inside the streams
    Case(508, 9, 6, 2, 1, 1, 0, 0, 0, 1, 1, ()),        # 32 workgroups, the last of 12 cells
    Case(512, 5, 2, 1, 0, 0, 256, 0, 0, 0, 0, ()),      # the largest supported
]


def case_id(c):
    return "C%d-S%d-T%d-d%d%s%s%s%s%s%s%s" % (c.C, c.S, c.T, c.ndir, "-cifg" if c.cifg else "", "-ragged" if c.ragged else "",
                                             "-kf%d@%d" % (c.k_first, c.col_first) if c.k_first else "", "-skip" if c.skip else "",
                                             "" if c.gp else "-nogp", "-dmax" if c.dmax else "", "-win" if c.windows else "")


def gates_of(c):
    return 3 if c.cifg else 4


def launches(c):
    return c.windows if c.windows else ((0, 0),)


def build_case(c):
    """Seeded inputs of a case, float32, in the padded layout the launch gets: ld = (G+3) C + 8, ldw = C + 4, grad_ld = C + 4, ldw_first =
    k_first + 4, every pad column holding CANARY.  Scales: gate pre-activations and dL/dm 1, history 0.5, weights 0.08, peepholes 0.3."""
    G, Cc, S, T = gates_of(c), c.C, c.S, c.T
    W = (G + 3) * Cc
    rng = np.random.default_rng([c.C, c.S, c.T, c.ndir, c.cifg, c.ragged, c.k_first, c.col_first, c.skip])
    rnd = lambda *shape, scale=1.0: (rng.standard_normal(shape) * scale).astype(np.float32)
    inp = dict(case=c, ld=W + 8, ldw=Cc + 4, grad_ld=Cc + 4, ldw_first=c.k_first + 4, dirs=[])
    inp["lens"] = np.asarray([(0, 1, T, max(T - 1, 0))[s % 4] for s in range(S)], np.int32) if c.ragged else None
    for d in range(c.ndir):
        hist = T + 1 if d else 0
        y = np.zeros((T + 2, S, inp["ld"]), np.float32)      # what aslp_lstm_seq_fill leaves in the row blocks 0 and T+1; 1..T are set below
        y[1:T + 1, :, :G * Cc] = rnd(T, S, G * Cc)           # x-part + bias
        y[1:T + 1, :, G * Cc:W] = 0.0
        y[hist, :, G * Cc:W] = rnd(S, 3 * Cc, scale=0.5)     # c, h, m of the history
        if c.k_first:
            y[hist, :, c.col_first:c.col_first + c.k_first] = rnd(S, c.k_first, scale=0.5)   # r(0)
        y[:, :, W:] = CANARY
        dd = np.zeros((T + 2, S, inp["ld"]), np.float32)
        dd[1:T + 1, :, (G + 2) * Cc:W] = rnd(T, S, Cc)       # dL/dm from the layer above
        dd[:, :, W:] = CANARY
        w = np.full((G * Cc, inp["ldw"]), CANARY, np.float32)
        w[:, :Cc] = rnd(G * Cc, Cc, scale=0.08)
        wf = np.full((G * Cc, inp["ldw_first"]), CANARY, np.float32)
        wf[:, :c.k_first] = rnd(G * Cc, c.k_first, scale=0.08)
        inp["dirs"].append(dict(y=y, d=dd, w=w, w_first=wf, peep_i=rnd(Cc, scale=0.3), peep_f=rnd(Cc, scale=0.3), peep_o=rnd(Cc, scale=0.3),
                                reverse=d))
    return inp


# ---- the model ----------------------------------------------------------------------------------------------------------------------

def _sigm(x):
    e = np.exp(-np.abs(x))
    return np.where(x > 0, 1 / (1 + e), e / (1 + e)).astype(x.dtype)


def _cols(c):
    G, Cc = gates_of(c), c.C
    og, oi, of, oo = (0, None, Cc, 2 * Cc) if c.cifg else (0, Cc, 2 * Cc, 3 * Cc)
    return og, oi, of, oo, G * Cc, (G + 1) * Cc, (G + 2) * Cc


def forward(inp, d, dtype=np.float64):
    c, q = inp["case"], inp["dirs"][d]
    G, Cc, S, T = gates_of(c), c.C, c.S, c.T
    W = (G + 3) * Cc
    og, oi, of, oo, oc, oh, om = _cols(c)
    sl = lambda o: slice(o, o + Cc)
    y = q["y"][:, :, :W].astype(dtype)
    w, pi, pf, po = q["w"][:, :Cc].astype(dtype), q["peep_i"].astype(dtype), q["peep_f"].astype(dtype), q["peep_o"].astype(dtype)
    hist = T + 1 if q["reverse"] else 0
    r0 = q["y"][hist, :, c.col_first:c.col_first + c.k_first].astype(dtype)   # read before the loop stores anything
    for step in range(T):
        t = T - step if q["reverse"] else 1 + step
        tp = t + 1 if q["reverse"] else t - 1
        pre = y[t, :, :G * Cc].copy()
        if step == 0 and c.k_first:
            pre += r0 @ q["w_first"][:, :c.k_first].astype(dtype).T
        elif not (step == 0 and c.skip):
            pre += y[tp, :, sl(om)] @ w.T
        cp = y[tp, :, sl(oc)]
        g = np.tanh(pre[:, sl(og)])
        f = _sigm(pre[:, sl(of)] + cp * pf)
        if c.cifg:
            cc = -g * f + g + cp * f
        else:
            i = _sigm(pre[:, sl(oi)] + cp * pi)
            cc = g * i + cp * f
            y[t, :, sl(oi)] = i
        cc = np.clip(cc, -50, 50)
        h = np.tanh(cc)
        o = _sigm(pre[:, sl(oo)] + cc * po)
        y[t, :, sl(og)], y[t, :, sl(of)], y[t, :, sl(oo)] = g, f, o
        y[t, :, sl(oc)], y[t, :, sl(oh)], y[t, :, sl(om)] = cc, h, h * o
        if inp["lens"] is not None:
            y[t, t > inp["lens"], :] = 0
    return y


def backward(inp, d, y, dtype=np.float64):
    """y: the activations of direction d (row blocks 0 .. T+1, history included).  No masking of its own: the zeroed rows of y carry it."""
    c, q = inp["case"], inp["dirs"][d]
    G, Cc, S, T = gates_of(c), c.C, c.S, c.T
    W = (G + 3) * Cc
    og, oi, of, oo, oc, oh, om = _cols(c)
    sl = lambda o: slice(o, o + Cc)
    y = y.astype(dtype)
    dd = q["d"][:, :, :W].astype(dtype)
    w, pi, pf, po = q["w"][:, :Cc].astype(dtype), q["peep_i"].astype(dtype), q["peep_f"].astype(dtype), q["peep_o"].astype(dtype)
    dsigm = lambda yy, e: e * yy * (1 - yy)
    dtanh = lambda yy, e: e * (1 - yy * yy)
    for step in range(T):
        t = 1 + step if q["reverse"] else T - step
        tn = t - 1 if q["reverse"] else t + 1
        tp = t + 1 if q["reverse"] else t - 1
        dm = dd[t, :, sl(om)] + dd[tn, :, :G * Cc] @ w
        yo, yh, yg, yf = y[t, :, sl(oo)], y[t, :, sl(oh)], y[t, :, sl(og)], y[t, :, sl(of)]
        dh = dtanh(yh, dm * yo)
        do = dsigm(yo, dm * yh)
        dc = dd[t, :, sl(oc)] + dh
        dc = dd[tn, :, sl(oc)] * y[tn, :, sl(of)] + dc
        if not c.cifg:
            dc = dc + dd[tn, :, sl(oi)] * pi
        dc = dc + dd[tn, :, sl(of)] * pf
        dc = dc + do * po
        cp = y[tp, :, sl(oc)]
        if c.cifg:
            df = dsigm(yf, -dc * yg + dc * cp)
            dg = dtanh(yg, -dc * yf + dc)
        else:
            yi = y[t, :, sl(oi)]
            df = dsigm(yf, dc * cp)
            dd[t, :, sl(oi)] = dsigm(yi, dc * yg)
            dg = dtanh(yg, dc * yi)
        dd[t, :, sl(om)], dd[t, :, sl(oh)], dd[t, :, sl(oo)], dd[t, :, sl(oc)] = dm, dh, do, dc
        dd[t, :, sl(of)], dd[t, :, sl(og)] = df, dg
    return dd


def grad_partial(inp, d, y, dd, s_begin=0, s_count=0):
    """{chain index: [7, C]} of direction d for the launch over [s_begin, s_begin + s_count) (s_count == 0: all streams): chain = group *
    ndir + d, groups of 8 streams counted inside the window; rows d_g, d_i, d_f, d_o, d_i c(t-1), d_f c(t-1), d_o c(t) summed over the chain's
    streams and all timesteps (rows 1 and 4 are not formed with coupled gates: left zero here, never compared)."""
    c, q = inp["case"], inp["dirs"][d]
    Cc, T = c.C, c.T
    og, oi, of, oo, oc, oh, om = _cols(c)
    sl = lambda o: slice(o, o + Cc)
    ns = s_count if s_count > 0 else c.S
    cur = slice(1, T + 1)
    prev = slice(2, T + 2) if q["reverse"] else slice(0, T)
    out = {}
    for grp in range((ns + 7) // 8):
        ss = slice(s_begin + 8 * grp, s_begin + min(8 * grp + 8, ns))
        rows = np.zeros((7, Cc), np.float64)
        sm = lambda a: a.astype(np.float64).sum(axis=(0, 1))
        rows[0], rows[2], rows[3] = sm(dd[cur, ss, sl(og)]), sm(dd[cur, ss, sl(of)]), sm(dd[cur, ss, sl(oo)])
        rows[5] = sm(dd[cur, ss, sl(of)] * y[prev, ss, sl(oc)])
        rows[6] = sm(dd[cur, ss, sl(oo)] * y[cur, ss, sl(oc)])
        if not c.cifg:
            rows[1], rows[4] = sm(dd[cur, ss, sl(oi)]), sm(dd[cur, ss, sl(oi)] * y[prev, ss, sl(oc)])
        out[grp * c.ndir + d] = rows
    return out


def dmax(inp, dd):
    c = inp["case"]
    v = np.abs(np.asarray(dd)[1:c.T + 1, :, :gates_of(c) * c.C])
    v = v[np.isfinite(v)]
    return float(v.max()) if v.size else 0.0


def tensors(c, backward_pass):
    """(name, column offset) of what a pass leaves and the tests compare, C columns each"""
    og, oi, of, oo, oc, oh, om = _cols(c)
    names = [("g", og)] + ([] if c.cifg else [("i", oi)]) + [("f", of), ("o", oo), ("c", oc), ("h", oh)]
    return [("d_" + n, o) for n, o in names] if backward_pass else names + [("m", om)]


# ---- the launches ----------------------------------------------------------------------------------------------------------------------

def run_on_gpu(aslp, torch, dev, inp, split16, pieces, want_pieces):
    """Both passes of a case on the GPU under one pair of switches, through the C ABI: aslp_lstm_seq_fill, the gate pre-activations and the
    history, aslp_lstm_seq_forward, then aslp_lstm_seq_backward on what it left -- one launch per stream window.  Checks after every launch:
    the error state, aslp_lstm_seq_last_pieces / _last_dmax, and bit for bit everything the launch has no business writing (pad columns,
    streams outside the window, history row blocks, the inputs it only reads, grad_partial rows of inactive chains and of d_i with coupled
    gates, dmax_parts where none are formed).  Returns numpy copies: y, d per direction, grad_partial and dmax_parts per launch."""
    lib, c = aslp.lib, inp["case"]
    Seq = aslp._lib.Seq
    G, Cc, S, T, ld = gates_of(c), c.C, c.S, c.T, inp["ld"]
    W = (G + 3) * Cc
    same = lambda a, b: np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    a = Seq()
    a.ndir, a.ld, a.ldw, a.T, a.S, a.C, a.cifg = c.ndir, ld, inp["ldw"], T, S, Cc, c.cifg
    lens = to_dev(inp["lens"]) if inp["lens"] is not None else None
    dev_dirs = []
    for d, q in enumerate(inp["dirs"]):
        y = torch.zeros((T + 2) * S, ld, device=dev)
        lib.aslp_lstm_seq_fill(y.data_ptr(), ld, T, S, (G + 2) * Cc, Cc)       # before anything is stored into it
        hist = T + 1 if q["reverse"] else 0
        yv, y0 = y.view(T + 2, S, ld), to_dev(q["y"])
        yv[1:T + 1, :, :G * Cc] = y0[1:T + 1, :, :G * Cc]
        yv[hist] = y0[hist]
        yv[:, :, W:] = CANARY
        t = dict(y=y, d=to_dev(q["d"]).view((T + 2) * S, ld), w=to_dev(q["w"]), w_first=to_dev(q["w_first"]),
                 peep_i=to_dev(q["peep_i"]), peep_f=to_dev(q["peep_f"]), peep_o=to_dev(q["peep_o"]))
        p = a.dir[d]
        p.y, p.d, p.w, p.peep_i, p.peep_f, p.peep_o = (t[k].data_ptr() for k in ("y", "d", "w", "peep_i", "peep_f", "peep_o"))
        p.seq_lengths = lens.data_ptr() if lens is not None else None
        p.reverse, p.skip_first_product = q["reverse"], c.skip
        if c.k_first:
            assert lib.aslp_lstm_seq_first_product_supported_for(c.k_first, Cc) == 1, (c.k_first, Cc)
            p.w_first, p.ldw_first, p.k_first, p.col_first = t["w_first"].data_ptr(), inp["ldw_first"], c.k_first, c.col_first
        dev_dirs.append(t)
    part = torch.full((8 * 7, inp["grad_ld"]), CANARY, device=dev)
    dmx = [torch.full((256,), CANARY, device=dev) for _ in range(2)]
    if c.gp:
        a.grad_partial, a.grad_ld = part.data_ptr(), inp["grad_ld"]
    if c.dmax:
        for d in range(c.ndir):
            a.dmax_parts[d] = dmx[d].data_ptr()
    readonly = lambda: [t[k].cpu().numpy() for t in dev_dirs for k in ("w", "w_first", "peep_i", "peep_f", "peep_o")]
    ro0 = readonly()
    out = dict(parts=[], dmax=[], last_dmax=[])
    lib.aslp_lstm_split16(split16)
    aslp.ops.set_lstm_operand_pieces(pieces)
    try:
        if c.windows:
            assert lib.aslp_lstm_seq_supported(C.byref(a), 0) == (1 if S <= 64 // c.ndir else 0)
        for backward_pass, buf in ((0, "y"), (1, "d")):
            y_before_bwd = [t["y"].cpu().numpy() for t in dev_dirs]
            for s_begin, s_count in launches(c):
                a.s_begin, a.s_count = s_begin, s_count
                before = [t[buf].cpu().numpy().reshape(T + 2, S, ld) for t in dev_dirs]
                part.fill_(CANARY)
                assert lib.aslp_lstm_seq_supported(C.byref(a), backward_pass) == 1, (case_id(c), backward_pass, s_begin, s_count)
                (lib.aslp_lstm_seq_backward if backward_pass else lib.aslp_lstm_seq_forward)(C.byref(a))
                torch.cuda.synchronize()
                aslp._lib.check_error()
                assert lib.aslp_lstm_seq_last_pieces() == want_pieces, (case_id(c), lib.aslp_lstm_seq_last_pieces(), want_pieces)
                after = [t[buf].cpu().numpy().reshape(T + 2, S, ld) for t in dev_dirs]
                lo, hi = (s_begin, s_begin + s_count) if s_count else (0, S)
                for d, (b0, b1) in enumerate(zip(before, after)):
                    what = (case_id(c), buf, "direction", d, "window", s_begin, s_count)
                    assert same(b0[:, :, W:], b1[:, :, W:]), what + ("pad columns",)
                    assert same(b0[:, :lo], b1[:, :lo]) and same(b0[:, hi:], b1[:, hi:]), what + ("streams outside the window",)
                    assert same(b0[[0, T + 1]], b1[[0, T + 1]]), what + ("row blocks 0 and T+1",)
                for r0, r1 in zip(ro0, readonly()):
                    assert same(r0, r1), (case_id(c), "an input the launch only reads")
                if backward_pass:
                    for d, t in enumerate(dev_dirs):
                        assert same(y_before_bwd[d], t["y"].cpu().numpy()), (case_id(c), "the backward pass wrote into y", d)
                    pn, nd = part.cpu().numpy().reshape(8, 7, inp["grad_ld"]), lib.aslp_lstm_seq_last_dmax()
                    nchains = c.ndir * (((s_count or S) + 7) // 8)
                    assert np.all(pn[:, :, Cc:] == CANARY) and np.all(pn[nchains:] == CANARY), (case_id(c), "grad_partial pad / inactive chains")
                    if c.cifg or not c.gp:
                        assert np.all(pn[:, [1, 4]] == CANARY) and (c.gp or np.all(pn == CANARY)), (case_id(c), "grad_partial rows nobody forms")
                    wpc = (Cc + 15) // 16
                    assert nd == (8 * wpc if (c.dmax and want_pieces and not c.windows) else 0), (case_id(c), "last_dmax", nd)
                    dn = [v.cpu().numpy() for v in dmx]
                    for d in range(2):   # (a windowed launch of the fp16 kernels may leave its own workgroups' maxima: incomplete, so not announced)
                        assert np.all(dn[d][8 * wpc:] == CANARY) and (want_pieces and c.dmax or np.all(dn[d] == CANARY)), (case_id(c), "dmax_parts nobody forms", d)
                    out["parts"].append(pn[:nchains, :, :Cc].copy())
                    out["dmax"].append([v[:nd].copy() for v in dn])
                    out["last_dmax"].append(nd)
            out[buf] = [t[buf].cpu().numpy().reshape(T + 2, S, ld)[:, :, :W].copy() for t in dev_dirs]
    finally:
        lib.aslp_lstm_split16(-1)
        aslp.ops.set_lstm_operand_pieces(-1)
    return out


def errors(got, ref):
    """(relative l2 error, largest element error relative to max(1, largest |reference|)) of one tensor against its float64 reference"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    den = np.linalg.norm(ref)
    l2 = np.linalg.norm(got - ref)
    return float(l2 / den if den > 0 else l2), float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max())) if ref.size else 0.0


def compare(inp, got, ref_y, ref_d, ref_parts, bar):
    """Every tensor of every direction and every grad_partial row of every active chain against the model; returns the worst (l2, element)
    pair seen, after asserting each below (bar, 10 bar).  ref_parts: per launch {chain: [7, C]}."""
    c = inp["case"]
    worst = [0.0, 0.0]
    fails = []

    def one(what, a, b):
        if not np.isfinite(a).all():
            fails.append(what + ("not finite",))
            return
        l2, el = errors(a, b)
        worst[0], worst[1] = max(worst[0], l2), max(worst[1], el)
        if not (l2 < bar and el < 10 * bar):
            fails.append(what + (l2, el))

    served = np.zeros(c.S, bool)   # the streams some launch of the pass served: all of them unless the windows leave some out
    for s_begin, s_count in launches(c):
        served[s_begin:s_begin + (s_count or c.S)] = True
    for d in range(c.ndir):
        for backward_pass, g, r in ((0, got["y"][d], ref_y[d]), (1, got["d"][d], ref_d[d])):
            for name, off in tensors(c, backward_pass):
                one((case_id(c), "direction", d, name), g[1:c.T + 1, served, off:off + c.C], r[1:c.T + 1, served, off:off + c.C])
    if c.gp:
        for k, chains in enumerate(ref_parts):
            for chain, rows in chains.items():
                for row in range(7):
                    if not (c.cifg and row in (1, 4)):
                        one((case_id(c), "launch", k, "grad_partial chain", chain, "row", row), got["parts"][k][chain, row], rows[row])
    assert not fails, fails
    return tuple(worst)


def as_got(c, ys, ds, parts):
    """a model run in the shape run_on_gpu returns (for compare)"""
    dense = []
    for chains in parts:
        a = np.zeros((max(chains) + 1, 7, c.C))
        for chain, rows in chains.items():
            a[chain] = rows
        dense.append(a)
    return dict(y=ys, d=ds, parts=dense)


def reference(inp, dtype=np.float64):
    """(y per direction, d per direction, grad_partial per launch) of the model"""
    c = inp["case"]
    ys = [forward(inp, d, dtype) for d in range(c.ndir)]
    ds = [backward(inp, d, ys[d], dtype) for d in range(c.ndir)]
    parts = []
    for s_begin, s_count in launches(c):
        chains = {}
        for d in range(c.ndir):
            chains.update(grad_partial(inp, d, ys[d], ds[d], s_begin, s_count))
        parts.append(chains)
    return ys, ds, parts
