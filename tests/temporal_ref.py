"""Float64 models of RowConvolution and CompactFsmn (the definitions in the comments of csrc/temporal.hip and oracle/aslp_oracle_temporal.c),
the element-wise bars that any fp32 evaluation of them keeps, and the case tables of tests/test_temporal_kernels_gpu.py (checked on a
machine without GPU by tests/test_temporal_ref_cpu.py, which also holds the oracle to the same bars).

THE BAR is derived, never measured: an fp32 sum of n products, in any order, with or without FMA, in one pass or by partial sums, lies within
    gamma_m * A,   gamma_m = m u / (1 - m u),   u = 2^-24,   A = sum |a_i| |b_i|
of the exact sum (Higham, Accuracy and Stability of Numerical Algorithms, (3.5) and section 4.2: a product costs one rounding, an addition tree
of n leaves at most n - 1 on any path), with m = n + (the further fp32 roundings on the way to that output).  Adding an exact zero (an empty
accumulator, a tap beyond K with weight 0, a partial sum of a chunk without frames) rounds nothing, so n counts the terms of the DEFINITION.
A missing, doubled or misplaced term is an error of the size |a| |b| ~ A / n, a factor 1 / (n gamma_n) ~ 2^24 / n^2 above the bar.

m per output (EXTRA_ROUNDINGS below is m - n):
    rowconv out      n = K + 1 (0 past L)             m = n      a plain sum of products
    rowconv in_diff  n = min(K, t) + 1 (0 past L)     m = n      a plain sum of products
    rowconv w_diff   n = sum_s L_s                    m = n      partial sums per (chunk, stream group), then their sum: still one tree
    fsmn out         n = the taps j with t + j - P in [0, T)   m = n + 1   the sum of products, then src + sum; A includes |src|
    fsmn in_diff     n = the taps j with t + j - F in [0, T)   m = n + 1   likewise with out_diff
    fsmn corr        n = the frames t with t + i - P in [0, T) m = n      partial sums per chunk, then their sum; clip rounds nothing
Where n = 0 the bar is 0: zeros past a stream's length are exact.

STEPPED PARAMETERS.  With g' = the computed gradient, |g' - g| <= B:
    rowconv  c' = fl(mmt c + g')  (one rounding fused, two as scale + axpy):      |c' - c_new| <= Bc = B + 3u (|mmt c| + |g| + B)
             w' = fl(w + fl(-lr c'))  (two roundings, one fused):                 |w' - w_new| <= lr Bc + 3u (|w| + lr (|c_new| + Bc))
    fsmn     coef' = fl(coef + fl(-lr corr'))                                     |coef' - coef_new| <= lr B + 3u (|coef| + lr (|corr_new| + B))
(each rounding contributes u times at most the sum of the magnitudes it sees, which the parentheses bound; 3u covers two roundings and the
second-order terms).  lr and mmt are the fp32 numbers the kernels receive (LR, MMT below), exact in float64.

CLIP (CompactFsmn, clip > 0).  clip() is 1-Lipschitz, so |corr' - clip(g)| <= B everywhere; besides, an element with |g| - B > clip IS
+-clip bit for bit (and its share of the step's bar is 0), one with |g| + B < clip is held to B, and one in between may be either.

STATE.  A case makes two consecutive calls, and the second starts from the parameters (and momentum buffer) the first left.  The model of a
call starts from the fp32 state the implementation under test holds before it -- read back, exact in float64 -- so every bar above speaks
of ONE call and needs no allowance for the error of the call before, while momentum and step are still judged from a state that is not zero.
"""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
SENTINEL = -7.25
LR = float(np.float32(0.01))
MMT = float(np.float32(0.9))
EXTRA_ROUNDINGS = {"rc_out": 0, "rc_in_diff": 0, "rc_w_diff": 0, "fsmn_out": 1, "fsmn_in_diff": 1, "fsmn_corr": 0}

# per element: the float64 value, the bar, and for a sum of products the number of terms n and the sum A of their magnitudes
Out = namedtuple("Out", "v bar n A", defaults=(None, None))
f64 = lambda a: np.asarray(a, np.float64)


def gamma(m):
    m = f64(m)
    return m * U / (1.0 - m * U)


def bar_of(key, n, A):
    return gamma(np.where(n > 0, n + EXTRA_ROUNDINGS[key], 0)) * A


def summed(key, v, n, A, shape=None):
    """an output that is a sum of n products of magnitudes A, with its bar"""
    v, n, A = (a.reshape(shape) if shape else a for a in (v, n, A))
    return Out(v, bar_of(key, n, A), n, A)


def step_bar(w_old, lr, c_new, Bc):
    """|fl(w_old + fl(-lr c')) - (w_old - lr c_new)| for |c' - c_new| <= Bc"""
    return lr * Bc + 3 * U * (np.abs(w_old) + lr * (np.abs(c_new) + Bc))


# ---- RowConvolution ---------------------------------------------------------------------------------------------------------------------
def rowconv_model(w, w_corr, x, od, T, S, lens, lr=LR, mmt=MMT):
    """one call (forward, backward, step): w, w_corr [D x (K+1)] the fp32 state before it; x, od [T*S x D], row t*S + s.
    -> {out, in_diff, w_diff, w_corr, w: Out}"""
    w, w_corr = f64(w), f64(w_corr)
    D, K1 = w.shape
    x, od = f64(x).reshape(T, S, D), f64(od).reshape(T, S, D)
    L = np.minimum(np.asarray(lens, np.int64), T)
    out, A_out, n_out = np.zeros((T, S, D)), np.zeros((T, S, D)), np.zeros((T, S, D), np.int64)
    idf, A_idf, n_idf = np.zeros((T, S, D)), np.zeros((T, S, D)), np.zeros((T, S, D), np.int64)
    g, A_g = np.zeros((D, K1)), np.zeros((D, K1))
    wt = w.T[None]   # [1, K+1, D]
    for s in range(S):
        Ls = int(L[s])
        if Ls <= 0:
            continue   # an empty stream: zeros, and no share in the gradient
        rows = np.minimum(np.arange(Ls)[:, None] + np.arange(K1)[None, :], Ls - 1)   # the last frame repeats
        xs = x[rows, s, :]   # [Ls, K+1, D]
        out[:Ls, s] = (xs * wt).sum(1)
        A_out[:Ls, s] = (np.abs(xs) * np.abs(wt)).sum(1)
        n_out[:Ls, s] = K1
        g += np.einsum("tkd,td->dk", xs, od[:Ls, s])
        A_g += np.einsum("tkd,td->dk", np.abs(xs), np.abs(od[:Ls, s]))
        for k in range(min(K1, Ls)):   # what falls on the replicated tail is dropped
            idf[k:Ls, s] += w[:, k] * od[:Ls - k, s]
            A_idf[k:Ls, s] += np.abs(w[:, k]) * np.abs(od[:Ls - k, s])
            n_idf[k:Ls, s] += 1
    n_g = np.full((D, K1), int(L.clip(0).sum()))
    w_diff = summed("rc_w_diff", g, n_g, A_g)
    B = w_diff.bar
    c_new = mmt * w_corr + g
    Bc = B + 3 * U * (np.abs(mmt * w_corr) + np.abs(g) + B)
    return dict(out=summed("rc_out", out, n_out, A_out, (T * S, D)), in_diff=summed("rc_in_diff", idf, n_idf, A_idf, (T * S, D)),
                w_diff=w_diff, w_corr=Out(c_new, Bc), w=Out(w - lr * c_new, step_bar(w, lr, c_new, Bc)))


# ---- CompactFsmn ------------------------------------------------------------------------------------------------------------------------
def _fir(src, taps, pad):
    """v[t] = src[t] + sum_j taps[j] src[t + j - pad], rows outside [0, T) count as 0; -> (v, A, n)"""
    T, D = src.shape
    v, A, n = src.copy(), np.abs(src), np.zeros((T, D), np.int64)
    for j in range(taps.shape[0]):
        lo, hi = max(0, pad - j), min(T, T + pad - j)   # t + j - pad in [0, T)
        if lo < hi:
            v[lo:hi] += taps[j] * src[lo + j - pad:hi + j - pad]
            A[lo:hi] += np.abs(taps[j]) * np.abs(src[lo + j - pad:hi + j - pad])
            n[lo:hi] += 1
    return v, A, n


def fsmn_grad(x, od, P, F):
    """the unclipped tap gradient g[i] = sum_t x[t + i - P] od[t]; -> (g, A, n)"""
    x, od = f64(x), f64(od)
    T, D = x.shape
    C = P + F + 1
    g, A, n = np.zeros((C, D)), np.zeros((C, D)), np.zeros((C, D), np.int64)
    for i in range(C):
        lo, hi = max(0, P - i), min(T, T + P - i)
        if lo < hi:
            g[i] = (x[lo + i - P:hi + i - P] * od[lo:hi]).sum(0)
            A[i] = (np.abs(x[lo + i - P:hi + i - P]) * np.abs(od[lo:hi])).sum(0)
            n[i] = hi - lo
    return g, A, n


def fsmn_model(coef, x, od, P, F, clip=0.0, lr=LR):
    """one call: coef [(P+F+1) x D] the fp32 state before it.  -> {out, in_diff, corr, coef: Out} and, with clip > 0, `sure` (the elements
    that must be +-clip exactly: +1 / -1) and `either` (the elements that may be clipped or not)"""
    coef, x, od = f64(coef), f64(x), f64(od)
    out, A_out, n_out = _fir(x, coef, P)
    idf, A_idf, n_idf = _fir(od, coef[::-1], F)
    g, A_g, n_g = fsmn_grad(x, od, P, F)
    r = dict(out=summed("fsmn_out", out, n_out, A_out), in_diff=summed("fsmn_in_diff", idf, n_idf, A_idf), g=summed("fsmn_corr", g, n_g, A_g))
    B = r["g"].bar
    if clip > 0.0:
        sure = np.where(np.abs(g) - B > clip, np.sign(g), 0.0)
        r["sure"], r["either"] = sure, (sure == 0) & ~(np.abs(g) + B < clip)
        corr = np.clip(g, -clip, clip)
        B = np.where(sure != 0, 0.0, B)
    else:
        corr = g
    r["corr"] = Out(corr, B, n_g, A_g)
    r["coef"] = Out(coef - lr * corr, step_bar(coef, lr, corr, B) if lr != 0.0 else np.zeros_like(coef))
    return r


# ---- judging ----------------------------------------------------------------------------------------------------------------------------
def check(got, want, what, fails):
    """|got - want.v| <= want.bar element by element (bar 0: exactly); -> the largest err / bar"""
    got = f64(got).reshape(want.v.shape)
    err = np.abs(got - want.v)
    bad = ~(err <= want.bar)   # (a NaN is bad)
    if bad.any():
        i = np.unravel_index(int(np.argmax(np.where(bad, np.where(np.isnan(err), np.inf, err - want.bar), -1.0))), err.shape)
        fails.append("%s: %d of %d elements outside their bar; worst at %s: got %.9g, float64 %.9g, bar %.3g" %
                     (what, int(bad.sum()), bad.size, i, got[i], want.v[i], want.bar[i]))
    pos = want.bar > 0
    return float((err[pos] / want.bar[pos]).max()) if pos.any() else 0.0


def check_clip(got, r, clip, what, fails):
    """the exact part of the clip rule: an element that must be clipped is +-clip bit for bit (clip is an fp32 number)"""
    got = f64(got).reshape(r["sure"].shape)
    bad = (r["sure"] != 0) & (got != r["sure"] * clip)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        fails.append("%s: %d elements beyond the clip are not +-%.9g; first at %s: %.9g (unclipped float64 %.9g)" % (what, int(bad.sum()), clip, i, got[i], r["g"].v[i]))


# ---- the host rules of csrc/temporal.hip, restated once (the real ones: aslp_rowconv_path / aslp_fsmn_path, asserted on the GPU) -----------
RC_CHUNK = 64          # frames per chunk of the streaming kernels
RC_COLS = 128          # columns per strip (two per lane)
RC_STREAMS = 4         # streams per workgroup
FSMN_FRAMES, FSMN_SPARE, FSMN_LDS_ROWS = 32, 24, 512


def rc_ring(K):
    """ring length of the streaming kernels at K + 1 taps; 0: the plain kernels"""
    return 21 if K + 1 == 21 else next((r for r in (4, 8, 16, 32) if K + 1 <= r), 0)


def rc_path(D, K, lds=(), offsets=()):
    """lds: the leading dimensions of the matrices of the call; offsets: whether each starts 4 bytes off an 8-byte boundary"""
    return rc_ring(K) if D % 2 == 0 and not any(ld % 2 for ld in lds) and not any(offsets) else 0


def fsmn_forward_tiled(C):
    return FSMN_FRAMES + C - 1 + FSMN_SPARE + C + FSMN_SPARE <= FSMN_LDS_ROWS        # C <= 216


def fsmn_backward_fused(C):
    return 2 * (FSMN_FRAMES + C - 1 + FSMN_SPARE) + C + FSMN_SPARE <= FSMN_LDS_ROWS  # C <= 126


# ---- case tables --------------------------------------------------------------------------------------------------------------------------
# odd: which matrix gets an odd leading dimension ("x": in, "od": out_diff, "y": out and in_diff); offset: `in` starts 4 bytes off an 8-byte
# boundary; one_sided: the case has no stream with L = T beside one with L < T, and says why
RcCase = namedtuple("RcCase", "name D K T S lens odd offset one_sided")


def _rc(name, D, K, T, S, lens, odd="", offset=False, one_sided=""):
    assert len(lens) == S and all(0 <= l <= T for l in lens)
    return RcCase(name, D, K, T, S, tuple(lens), odd, offset, one_sided)


RC_CASES = [
    # ring <4>: K = 0, 2, 3
    _rc("k0-one-frame", 2, 0, 1, 1, [1], one_sided="T = 1, S = 1"),
    _rc("k2", 126, 2, 63, 4, [63, 1, 62, 30]),
    _rc("k3-s5", 128, 3, 64, 5, [64, 63, 1, 33, 64]),                     # second stream group: three of its four streams are past S
    _rc("k2-ten-strips", 130, 2, 5, 20, [5, 4, 1, 3, 5] * 4),              # 2 column strips x 5 stream groups
    _rc("k3-empty-stream", 4, 3, 10, 4, [10, 0, 7, 1]),                    # L = 0: the oracle is not consulted for that stream
    # ring <8>: K = 4, 7
    _rc("k4", 130, 4, 65, 4, [65, 64, 1, 65]),
    _rc("k7-t60", 6, 7, 60, 4, [60, 58, 57, 1]),                           # backward (T + K = 67): 2 chunks, forward 1; L + K = 65 and 64
    # ring <16>: K = 8, 15
    _rc("k8", 4, 8, 130, 4, [130, 64, 65, 129]),
    _rc("k15-s1", 8, 15, 65, 1, [50], one_sided="S = 1; L + K = 65 is one row into the second chunk"),
    # ring <21, exact>: K = 20
    _rc("k20", 130, 20, 130, 5, [130, 129, 64, 65, 1]),
    # ring <32>: K = 16, 19, 21, 31
    _rc("k16", 2, 16, 64, 4, [64, 63, 48, 1]),                             # L + K = 64: the chunk edge itself
    _rc("k19", 6, 19, 65, 4, [65, 64, 46, 1]),                             # L + K = 65
    _rc("k21", 4, 21, 63, 5, [63, 62, 43, 44, 1]),
    _rc("k31", 128, 31, 130, 4, [130, 1, 98, 97]),                         # L + K = 129 and 128
    # the plain kernels
    _rc("k32", 4, 32, 65, 4, [65, 64, 33, 1]),
    _rc("k63", 2, 63, 64, 4, [64, 63, 1, 2]),                              # one group of 64 taps
    _rc("k64", 6, 64, 130, 5, [130, 129, 66, 65, 1]),                      # two groups
    _rc("odd-width", 65, 4, 65, 4, [65, 64, 1, 63]),
    _rc("odd-width-empty-stream", 3, 3, 10, 4, [10, 0, 7, 1]),
    _rc("odd-ld-in", 4, 7, 33, 4, [33, 32, 1, 20], odd="x"),
    _rc("odd-ld-out-diff", 4, 7, 33, 4, [33, 32, 1, 20], odd="od"),         # the forward (out, in) stays on ring <8>
    _rc("odd-ld-out", 4, 7, 33, 4, [33, 32, 1, 20], odd="y"),
    _rc("off-by-4-bytes", 4, 20, 33, 4, [33, 32, 1, 20], offset=True),
]
RC_BY_NAME = {c.name: c for c in RC_CASES}
RC_NAMES = [c.name for c in RC_CASES]


def rc_ld(case, which):
    """the leading dimension the tests give matrix `which` ("x", "od", "y") of a case: even unless the case (or the width) says otherwise"""
    return case.D + (3 if which in case.odd.split(",") and case.D % 2 == 0 else 4)


def rc_paths(case):
    """(forward, backward): ring length or 0"""
    lx, lod, ly = (rc_ld(case, m) for m in ("x", "od", "y"))
    return rc_path(case.D, case.K, (ly, lx), (False, case.offset)), rc_path(case.D, case.K, (ly, lx, lod), (False, case.offset, False))


RcInputs = namedtuple("RcInputs", "case w w_corr x od lens")


def rc_inputs(case):
    rng = np.random.default_rng(1000 + RC_NAMES.index(case.name))
    n = case.T * case.S
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    return RcInputs(case, f(case.D, case.K + 1), f(case.D, case.K + 1), [f(n, case.D) for _ in range(2)], [f(n, case.D) for _ in range(2)],
                    np.array(case.lens, np.int32))


FsmnCase = namedtuple("FsmnCase", "name D P F T clip")
_f = lambda D, P, F, T, clip=False: FsmnCase("d%d-p%d-f%d-t%d%s" % (D, P, F, T, "-clip" if clip else ""), D, P, F, T, clip)
FSMN_CASES = [
    _f(1, 0, 0, 1), _f(63, 0, 5, 31), _f(64, 5, 0, 32),                   # one-sided and minimal
    _f(65, 3, 3, 33), _f(8, 4, 3, 33), _f(8, 4, 4, 40),                    # C = 7, 8, 9: the ring block's edge
    _f(5, 10, 2, 4),                                                       # T < P
    _f(66, 32, 31, 70), _f(66, 32, 32, 70),                                # C = 64, 65: the second round of taps
    _f(66, 36, 36, 70), _f(66, 37, 36, 70),                                # C = 73, 74: 104 and 105 in-rows of the fused backward
    _f(66, 63, 62, 70), _f(66, 63, 63, 70),                                # C = 126, 127: fused | separate backward
    _f(66, 108, 107, 70), _f(66, 108, 108, 70),                            # C = 216, 217: tiled | plain forward
    _f(8, 1, 1, 1024), _f(8, 1, 1, 1025), _f(8, 1, 1, 2081),               # 32, 33 and 66 chunks: one, two and three rounds of the finish
    _f(66, 30, 30, 70, True), _f(66, 65, 64, 70, True),                    # clip on the fused (C = 61) and on the separate (C = 130) backward
]
FSMN_BY_NAME = {c.name: c for c in FSMN_CASES}
FSMN_NAMES = [c.name for c in FSMN_CASES]

FsmnInputs = namedtuple("FsmnInputs", "case coef x od clip")


def fsmn_inputs(case):
    """clip (per call): the median of |g|, as an fp32 number, or 0"""
    rng = np.random.default_rng(2000 + FSMN_NAMES.index(case.name))
    C = case.P + case.F + 1
    coef = ((rng.random((C, case.D)) - 0.5) * 0.6).astype(np.float32)
    x = [rng.standard_normal((case.T, case.D)).astype(np.float32) for _ in range(2)]
    od = [rng.standard_normal((case.T, case.D)).astype(np.float32) for _ in range(2)]
    clip = [float(np.float32(np.median(np.abs(fsmn_grad(x[k], od[k], case.P, case.F)[0])))) if case.clip else 0.0 for k in range(2)]
    return FsmnInputs(case, coef, x, od, clip)


def fsmn_paths(case):
    """(forward tiled, backward fused)"""
    C = case.P + case.F + 1
    return fsmn_forward_tiled(C), fsmn_backward_fused(C)
