"""Plain numpy float64 models of the BatchNormalization and Xent operations behind csrc/nn_fused.hip -- written from the definitions
(nnet-batch-normalization.h:177-284, nnet-loss.cc:63-122), not from the kernels or oracle/aslp_oracle.c -- and what the tests around
them share: the case tables with the instantiation every case must reach, the seeded inputs, the distances and the bars.

    bn_forward(x, scale, shift)            per-column mean and biased variance, inv_std = 1 / sqrt(var + 1e-7), xhat, out = xhat scale + shift,
                                           act = sigmoid(out); sum_x and sum_xx (the square rounded to fp32 first, :216-220) for the running sums
    bn_backward(x, fwd, od, scale, ...)    dy = od y (1 - y) with a folded Sigmoid; dshift = sum dy + mmt dshift0, dscale = sum xhat dy + mmt dscale0;
                                           in_diff by the reference's four steps (:238-276); D = dy scale, what the reference leaves in xhat
    bn_sequence(inp, has_y, step)          two consecutive forward + backward calls that carry the component's state (running sums, gradients
                                           and, with `step`, scale -= lr dscale, shift -= lr dshift; in_diff uses the scale from BEFORE the step)
    xent(y, t, fw, softmax)                optional row softmax, w = fw sum(t), diff = (y - t) w, the five sums with log(. + 1e-20), `correct` by
                                           the lowest-index arg-max of y and of t; a row whose targets sum to 0 is switched off (:80-85)

Everything is evaluated in float64 from the fp32 inputs.  MARGIN, the floors and the measured ratios: tests/test_bn_xent_kernels_gpu.py."""
import collections

import numpy as np

VAR_FLOOR = 1e-7
MMT, LR = float(np.float32(0.9)), float(np.float32(0.01))      # as the fp32 arguments the kernels and the oracle receive
SENTINEL = -7.25                                               # what a buffer holds where no call may write
# the GPU's distance to float64 may be MARGIN x the oracle's on the same output, with floors where fp32 is simply accurate:
# one rounding of the result (relative l2 2^-23) and four half-ulps of the largest element.  MARGIN is the smallest of 2, 3, 4 that is
# >= 1.3 x the worst ratio measured on an MI355X (2.10: tests/test_bn_xent_kernels_gpu.py MEASURED)
MARGIN = 3.0
FLOOR_L2, FLOOR_EL = 2.0 ** -23, 4 * 2.0 ** -24
PANEL_LANES, COOP_LANES, COOP_COLS = 64, 32, 32                # kPanelThreads / 4 column groups; kCoopLanes; kCoopCols

# ---- BatchNormalization: cases ---------------------------------------------------------------------------------------------------
BnCase = collections.namedtuple("BnCase", "name rows cols path q slots offset")   # path q slots: on a device with 256 CUs


def _bn(rows, cols, path, q=0, slots=0, offset=False):
    return BnCase("%s-%dx%d%s" % (path, rows, cols, "-offset" if offset else ""), rows, cols, path, q, slots, offset)


BN_CASES = [
    # three-launch (colreduce + write pass), one column per access: cols % 4 != 0
    _bn(7, 5, "three"), _bn(100, 37, "three"),
    # three-launch, 16-byte accesses: cols % 16 != 0, or more rows than a panel holds
    _bn(129, 260, "three"), _bn(1025, 64, "three"),
    # a panel shape on views whose rows start 4 bytes off a 16-byte boundary (pointer + 4, stride 36): the panel must stand down
    _bn(64, 32, "three", offset=True),
    # bn_forward_panel<4, SLOTS> / bn_backward_panel<4, SLOTS, ., .>: 64 row lanes, SLOTS rows per thread -- 4: rows <= 256, 8: <= 512, 16: <= 1024
    _bn(1, 16, "panel", 1, 4), _bn(2, 16, "panel", 1, 4), _bn(64, 16, "panel", 1, 4), _bn(37, 48, "panel", 1, 4), _bn(65, 16, "panel", 1, 4),
    _bn(256, 16, "panel", 1, 4),
    _bn(257, 16, "panel", 1, 8), _bn(512, 48, "panel", 1, 8),
    _bn(513, 16, "panel", 1, 16), _bn(1000, 48, "panel", 1, 16), _bn(1024, 16, "panel", 1, 16),
    # bn_forward_coop<SLOTS> / bn_backward_coop<SLOTS, ., .>: Q = min(4, 256 / (cols / 32)) workgroups of 32 row lanes per panel, rp = ceil(rows / Q)
    _bn(253, 32, "coop", 4, 4), _bn(512, 64, "coop", 4, 4),          # rp = 64 (the last chunk 61 rows), 128
    _bn(513, 32, "coop", 4, 8), _bn(1024, 32, "coop", 4, 8),         # rp = 129 (the last chunk 126 rows), 256
    _bn(700, 2080, "coop", 3, 8),                                    # 65 panels: Q = 3, rp = 234, the last chunk 232 rows
    _bn(1024, 2080, "coop", 3, 16), _bn(1000, 2080, "coop", 3, 16),  # rp = 342 / 334, the last chunk 340 / 332 rows
    _bn(200, 2752, "coop", 2, 4),                                    # 86 panels: Q = 2, rp = 100
    _bn(1024, 2752, "coop", 2, 16),                                  # rp = 512: every slot of every thread holds a row
]
BN_BY_NAME = {c.name: c for c in BN_CASES}
BN_NAMES = [c.name for c in BN_CASES]
# aslp_bn_forward_stats: (rows, cols) -> the Q its host rule picks; cols % 32 == 0, partial last 32-row group where rows % 32 != 0
BN_STATS_SHAPES = [(100, 32), (250, 64), (500, 32), (1000, 2048), (1024, 32)]


def bn_path(rows, cols, num_cu=256):
    """(path, Q, slots) by the host's rule (bn_panel_shape / bn_coop_shape of csrc/nn_fused.hip) for 16-byte aligned operands"""
    if cols % 16 != 0 or rows > 16 * PANEL_LANES:
        return "three", 0, 0
    if cols % COOP_COLS == 0 and cols // COOP_COLS <= 256:
        q = min(4, num_cu // (cols // COOP_COLS))
        if q >= 2 and -(-rows // q) >= 64:
            return "coop", q, next(s for s in (4, 8, 16) if -(-rows // q) <= s * COOP_LANES)
    return "panel", 1, next(s for s in (4, 8, 16) if rows <= s * PANEL_LANES)


def bn_stats_q(rows, cols):
    """row chunks per column panel of bn_forward_stats_kernel (aslp_bn_forward_stats_p)"""
    p, q = cols // COOP_COLS, 1
    while q < 8 and p * q * 2 <= 1024 and (rows + 2 * q - 1) // (2 * q) >= 64:
        q *= 2
    while (rows + q - 1) // q > 4 * COOP_LANES:
        q *= 2
    return q


BnInputs = collections.namedtuple("BnInputs", "case x od scale shift dscale0 dshift0")


def bn_matrix(rng, rows, cols, call):
    """ordinary columns N(0.5, 2); column 0 at mean 100, std 1; column 1 one value (variance 0: inv_std = 1 / sqrt(floor)) -- a value whose
    multiples are exact in fp32, so that every fp32 evaluation of the column's mean gives the same number; column 2 zero; column 3
    with one outlier of 1e3"""
    x = (rng.standard_normal((rows, cols)) * 2 + 0.5).astype(np.float32)
    x[:, 0] = (rng.standard_normal(rows) + 100.0).astype(np.float32)
    x[:, 1] = np.float32(3.25 if call == 0 else -1.5)
    x[:, 2] = 0.0
    x[(rows // 2) if call == 0 else 0, 3] = 1e3
    return x


def bn_inputs(case, seed=None):
    rng = np.random.default_rng(1000 + BN_NAMES.index(case.name) if seed is None else seed)
    rows, cols = case.rows, case.cols
    x = [bn_matrix(rng, rows, cols, k) for k in range(2)]
    od = [rng.standard_normal((rows, cols)).astype(np.float32) for _ in range(2)]
    f = lambda a: a.astype(np.float32)
    return BnInputs(case, x, od, f(rng.uniform(0.5, 1.5, cols)), f(rng.standard_normal(cols)), f(rng.standard_normal(cols)), f(rng.standard_normal(cols)))


# ---- BatchNormalization: the model -------------------------------------------------------------------------------------------------
def sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def bn_forward(x, scale, shift):
    x32 = np.asarray(x, np.float32)
    x = x32.astype(np.float64)
    scale, shift = np.asarray(scale, np.float64), np.asarray(shift, np.float64)
    mean = x.mean(0)
    xm = x - mean
    var = (xm * xm).mean(0)
    inv_std = 1.0 / np.sqrt(var + VAR_FLOOR)
    xhat = xm * inv_std
    out = xhat * scale + shift
    return dict(mean=mean, inv_std=inv_std, xhat=xhat, out=out, act=sigmoid(out), sum_x=x.sum(0), sum_xx=(x32 * x32).astype(np.float64).sum(0))


def bn_backward(x, fwd, od, scale, dscale0, dshift0, has_y, mmt=MMT):
    x, od, scale = np.asarray(x, np.float64), np.asarray(od, np.float64), np.asarray(scale, np.float64)
    rows = x.shape[0]
    dy = od * fwd["act"] * (1.0 - fwd["act"]) if has_y else od
    dshift = dy.sum(0) + mmt * np.asarray(dshift0, np.float64)
    dscale = (fwd["xhat"] * dy).sum(0) + mmt * np.asarray(dscale0, np.float64)
    D = dy * scale                                                   # 1. XsharpO_ <- dy gamma
    xm, inv = x - fwd["mean"], fwd["inv_std"]
    dvar = -0.5 * inv ** 3 * (xm * D).sum(0)                         # 2. delta-var
    dmean = -inv * D.sum(0) - (2.0 / rows) * dvar * xm.sum(0)        # 3. delta-mean
    in_diff = D * inv + xm * (2.0 / rows) * dvar + dmean / rows      # 4.
    return dict(in_diff=in_diff, D=D, dscale=dscale, dshift=dshift)


BN_MATRICES = ("out", "xhat", "act", "in_diff", "D")
BN_FORWARD_KEYS = ("out", "xhat", "act", "mean", "inv_std", "acc_means", "acc_vars")
BN_BACKWARD_KEYS = ("in_diff", "D", "dscale", "dshift", "scale", "shift")


def bn_sequence(inp, has_y, step, cache=None):
    """-> [call 0, call 1]: every output of a forward + backward call; scale / shift are the values AFTER the call.  cache: forward results
    by (call, scale, shift), shared between the sequences of a case"""
    scale, shift = inp.scale.astype(np.float64), inp.shift.astype(np.float64)
    dscale, dshift = inp.dscale0.astype(np.float64), inp.dshift0.astype(np.float64)
    accm, accv = np.zeros(inp.case.cols), np.zeros(inp.case.cols)
    calls = []
    for k in range(2):
        key = (k, scale.tobytes(), shift.tobytes())
        fwd = cache.get(key) if cache is not None else None
        if fwd is None:
            fwd = bn_forward(inp.x[k], scale, shift)
            if cache is not None:
                cache[key] = fwd
        accm, accv = accm + fwd["sum_x"], accv + fwd["sum_xx"]
        bwd = bn_backward(inp.x[k], fwd, inp.od[k], scale, dscale, dshift, has_y)
        dscale, dshift = bwd["dscale"], bwd["dshift"]
        if step:
            scale, shift = scale - LR * dscale, shift - LR * dshift
        o = dict(out=fwd["out"], xhat=fwd["xhat"], mean=fwd["mean"], inv_std=fwd["inv_std"], acc_means=accm, acc_vars=accv, scale=scale, shift=shift)
        if has_y:
            o["act"] = fwd["act"]
        o.update(bwd)
        calls.append(o)
    return calls


# ---- Xent: cases -----------------------------------------------------------------------------------------------------------------------
XentCase = collections.namedtuple("XentCase", "name rows cols stride kernel")
XENT_MAX_GRID = 4096                    # 2 kMaxGrid workgroups: beyond, a workgroup takes a second row
STATS0 = np.array([8.0, 4.0, 2.5, 1.25, 0.5])    # what the five accumulators hold before a call


def xent_kernel(cols, aligned=True):
    """the instantiation xent_eval_impl picks: slots per thread (the smallest of 4 / 8 / 16 / 32 that covers the row with 256 threads) and
    the column map (16-byte accesses: cols % 4 == 0 and every row 16-byte aligned); past 8192 classes the streaming kernel"""
    if cols > 8192:
        return "wide"
    per = next(p for p in (4, 8, 16, 32) if -(-cols // 256) <= p)
    return "per%d-%s" % (per, "vec" if cols % 4 == 0 and aligned else "scalar")


def _x(rows, cols, stride=None):
    return XentCase("%dx%d%s" % (rows, cols, "-ld%d" % stride if stride else ""), rows, cols, stride, xent_kernel(cols, stride is None or stride % 4 == 0))


XENT_CASES = [
    _x(16, 10), _x(16, 1023),                   # per4-scalar
    _x(16, 128), _x(16, 1024),                  # per4-vec
    _x(8, 1025), _x(8, 1028), _x(8, 2048),      # per8-scalar, per8-vec x 2
    _x(8, 2049), _x(8, 3000), _x(8, 4096),      # per16-scalar, per16-vec x 2
    _x(5, 4097), _x(5, 8192),                   # per32-scalar, per32-vec
    _x(4, 8193), _x(4, 20000),                  # wide
    _x(4100, 8), _x(4100, 516),                 # rows > 4096: workgroups 0..3 take rows 4096..4099 as their second row
    _x(8, 1028, 1029),                          # per8-scalar at a width the 16-byte map would take: rows of 1029 floats are not 16-byte aligned
]
XENT_EXPECT = ["per4-scalar"] * 2 + ["per4-vec"] * 2 + ["per8-scalar", "per8-vec", "per8-vec", "per16-scalar", "per16-vec", "per16-vec",
                                                       "per32-scalar", "per32-vec", "wide", "wide", "per4-vec", "per4-vec", "per8-scalar"]
XENT_BY_NAME = {c.name: c for c in XENT_CASES}
XENT_NAMES = [c.name for c in XENT_CASES]
TARGETS = ("labels", "onehot", "soft")
ARGMAX_GAP = 1e-3


def softmax_supported(cols):
    return 512 < cols <= 8192


XentInputs = collections.namedtuple("XentInputs", "case logits post labels fw onehot soft")


def softmax(a):
    a = np.asarray(a, np.float64)
    e = np.exp(a - a.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def argmax_gap(p):
    """per row: (largest - second largest) / largest"""
    top = np.partition(np.asarray(p, np.float64), -2, axis=-1)[:, -2:]
    return (top[:, 1] - top[:, 0]) / top[:, 1]


def xent_inputs(case):
    """logits N(0, 3) and their posteriors rounded to fp32 (what the posteriors-in entry points are given); a row is drawn again until the
    float64 posteriors' largest and second-largest values -- of the softmax of the logits AND of the fp32 posteriors -- differ by more
    than ARGMAX_GAP relative, so that no rounding decides an arg-max.  Frame weights are multiples of 2^-10 in [0, 1] and every target
    row sums to exactly 0 or 1 in fp32: `frames` and `correct` are then exact in every evaluation."""
    rng = np.random.default_rng(2000 + XENT_NAMES.index(case.name))
    rows, cols = case.rows, case.cols
    logits = (rng.standard_normal((rows, cols)) * 3).astype(np.float32)
    for _ in range(100):
        post = softmax(logits).astype(np.float32)
        bad = np.flatnonzero((argmax_gap(softmax(logits)) <= 2 * ARGMAX_GAP) | (argmax_gap(post) <= 2 * ARGMAX_GAP))
        if bad.size == 0:
            break
        logits[bad] = (rng.standard_normal((bad.size, cols)) * 3).astype(np.float32)
    else:
        raise AssertionError("no clear arg-max after 100 draws")
    labels = rng.integers(0, cols, rows).astype(np.int32)
    labels[2::4] = post.argmax(1)[2::4]        # every fourth row is classified correctly
    labels[1], labels[3] = -1, cols            # outside [0, cols): the row is switched off
    if rows > XENT_MAX_GRID:                   # ... also in a row that is a workgroup's second
        labels[XENT_MAX_GRID + 1], labels[XENT_MAX_GRID + 2] = cols, -1
    fw = (rng.integers(0, 1025, rows) / 1024.0).astype(np.float32)
    fw[0] = 0.0
    onehot = np.zeros((rows, cols), np.float32)
    ok = np.flatnonzero((labels >= 0) & (labels < cols))
    onehot[ok, labels[ok]] = 1.0
    soft = onehot.copy()
    soft[1] = 0.0                               # a row of zeros (it is one already: label -1)
    soft[2] = 0.0
    soft[2, :2] = [0.25, 0.75]
    for r in ok[(ok >= 4) & (ok % 3 == 0)]:     # two classes share the row
        soft[r, labels[r]], soft[r, (labels[r] + 1) % cols] = 0.625, 0.375
    return XentInputs(case, logits, post, labels, fw, onehot, soft)


def xent(y, t, fw, use_softmax):
    """-> (diff, posteriors, the call's increments [frames, correct, loss, entropy, likelihood])"""
    post = softmax(y) if use_softmax else np.asarray(y, np.float64)
    t = np.asarray(t, np.float64)
    w = np.asarray(fw, np.float64) * t.sum(1)
    diff = (post - t) * w[:, None]
    tw = t * w[:, None]
    hit = post.argmax(1) == t.argmax(1)        # np.argmax: the lowest index among equals
    with np.errstate(divide="ignore"):
        sums = [w.sum(), (w * hit).sum(), -(tw * np.log(post + 1e-20)).sum(), -(tw * np.log(t + 1e-20)).sum(), (tw * post).sum()]
    return diff, post, np.array(sums)


# ---- distances and bars ------------------------------------------------------------------------------------------------------------------
def rel_l2(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    den = np.linalg.norm(ref)
    return float(np.linalg.norm(a - ref) / den) if den > 0 else float(np.linalg.norm(a - ref))


# BatchNormalization outputs are measured over all columns and per column group: the oracle's fp32 mean leaves 1e-4 on the column at mean
# 100 and 7.5e-4 of noise on the column of one value (test_bn_xent_ref_cpu.ORACLE_CAP), and a bar taken over all columns at once lets an
# error of that size through on every ordinary column.  The GPU file holds matrices to the oracle's distance on `all` and on `rest`; the
# groups of one and two columns are printed only (the quotient of two single roundings says nothing).
BN_GROUPS = (("all", slice(None)), ("mean100", slice(0, 1)), ("flat", slice(1, 3)), ("rest", slice(3, None)))


def group_dist(e2, r2, em, rm, rows):
    """per column: squared error and squared reference summed over the rows, largest |error| and largest |reference| -> per column group
    (relative l2, largest error over max(1, largest |reference|): oracle_lib.max_err).  Where the reference is all zero (xhat of the flat
    columns) the l2 distance is the root mean square error: relative to elements of size 1."""
    out = {}
    for g, s in BN_GROUPS:
        num, den = float(np.sqrt(e2[s].sum())), float(np.sqrt(r2[s].sum()))
        out[g] = (num / den if den > 0 else num / float(np.sqrt(rows * len(e2[s]))), float(em[s].max()) / max(1.0, float(rm[s].max())))
    return out


def col_dist(a, ref):
    """distances of a matrix (or of a vector with one entry per column) per column group"""
    a, ref = np.atleast_2d(np.asarray(a, np.float64)), np.atleast_2d(np.asarray(ref, np.float64))
    d = a - ref
    return group_dist((d * d).sum(0), (ref * ref).sum(0), np.abs(d).max(0), np.abs(ref).max(0), a.shape[0])


def bar(d_ref, margin=None):
    """the (relative l2, largest element) distances to float64 allowed on an output whose oracle distances are d_ref"""
    m = MARGIN if margin is None else margin
    return max(m * d_ref[0], FLOOR_L2), max(m * d_ref[1], FLOOR_EL)


def ratio(d, d_ref):
    """the margin an output needs: its distance over the oracle's, on the measures where it lies above the floor (below it fp32 is simply
    accurate and the quotient of two roundings says nothing: 0).  Inside the bar <=> ratio <= MARGIN."""
    out = 0.0
    for a, b, f in zip(d, d_ref, (FLOOR_L2, FLOOR_EL)):
        if not a <= f:
            out = max(out, a / b if b > 0 else float("inf"))
    return out
