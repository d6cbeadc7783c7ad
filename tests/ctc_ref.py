"""A plain numpy float64 model of the CTC loss behind include/aslp_ctc.h (compute_ctc_loss, aslp_ctc_loss_strided, aslp_eesen_ctc_mseq) --
written from the definition of the loss, not from csrc/ctc.hip or oracle/aslp_oracle_ctc.c -- and what the tests around it share: the
seeded case list, the distances, and the thread rung / slot count that ctc_lattice_kernel takes for a minibatch.

    reference(acts, labels, in_len)   -> (costs [mb], grads [maxT, mb, A]), float64
        log-softmax over the alphabet; alpha and beta over ALL S = 2 L + 1 states of every frame (no [start, end) window: a state no
        alignment reaches simply holds -inf); per frame the products alpha beta reduced by label with np.logaddexp;
        grad = p - exp(out - log p - log Z).  An utterance with T <= 0 or L + repeats > T has cost 0 and zero rows; rows t >= T are zero.
        probs=True: `acts` are post-softmax outputs (the Eesen convention), used as they are.
    closed_form_cost(acts, n, mb, path) the cost of an utterance with exactly one alignment, -sum_t log p_t(path_t): no lattice involved

Inputs of a case: activations N(0, 1), + PEAK on the logits of one valid alignment (the labels, a blank between repeated labels, then
blanks up to T).  Without the peak (N(0, 1) x 2) the fp32 lattice of the oracle lies 7e-3 from float64 at L = 1792; with it the
posteriors are concentrated as in a trained network and the distance stays at 1e-3, while every label state is the favoured one at some
frame.  T = L + repeats + slack unless the utterance gives T itself."""
import collections

import numpy as np

PEAK = 4.0
LAT_SLOTS = 8             # kLatSlots of csrc/ctc.hip
# distance of an fp32 CTC to float64 that the GPU tests accept: MARGIN x the oracle's own distance on the same utterance, and floors
# where fp32 is simply accurate.  Two fp32 evaluations of one recursion that differ in a few roundings land at distances of the same
# order, not at the same distance: the margin started at 4 and, every ratio measured on an MI355X being <= 1.5 (compute_ctc_loss 1.00,
# aslp_eesen_ctc_mseq 1.47: tests/test_ctc_edges_gpu.py MEASURED), stands at 2.
MARGIN = 2.0
FLOOR_L2, FLOOR_EL, FLOOR_COST = 2e-5, 1e-5, 2e-6
# what tests/test_ctc_ref_cpu.py holds the oracle to on every utterance of every case, so that MARGIN x its distance stays a real bar
CAP_REF_L2, CAP_REF_COST = 5e-3, 5e-6

Utt = collections.namedtuple("Utt", "L slack T")          # T = None: L + repeats + slack
Case = collections.namedtuple("Case", "name group A utts seed")


def _u(L, slack=0, T=None):
    return Utt(L, slack, T)


CASES = [
    # thread rungs of ctc_lattice_kernel (64, 128, 256, 512 from the longest S), a short utterance beside the long ones
    Case("rungs-64", "rungs", 7, (_u(0, 3), _u(1, 9), _u(30, 0), _u(31, 1)), 11),            # S <= 63
    Case("rungs-128", "rungs", 7, (_u(2, 1), _u(32, 3), _u(33, 9), _u(63, 0)), 12),          # S = 65: the first 128-thread size; 127
    Case("rungs-256", "rungs", 7, (_u(5, 0), _u(64, 1), _u(65, 3), _u(127, 9)), 13),         # S = 129, 131, 255
    Case("rungs-512", "rungs", 7, (_u(1, 9), _u(128, 0), _u(129, 1), _u(255, 3)), 14),       # S = 257, 259, 511: one slot of 512 threads
    # slot counts 2..8 at both ends of every slot: L = 256 k -> S = 512 k + 1 (thread 0 alone in the last slot), L = 256 k - 1 -> S = 512 k - 1
    Case("slots-2-4", "slots", 12, (_u(256, 3), _u(511, 0), _u(512, 1), _u(767, 9), _u(768, 0)), 21),
    Case("slots-4-6", "slots", 12, (_u(1023, 1), _u(1024, 3), _u(1279, 0), _u(1280, 9)), 22),
    Case("slots-6-8", "slots", 12, (_u(1535, 9), _u(1536, 0), _u(1791, 3), _u(1792, 1), _u(2047, 0), _u(3, 1)), 23),
    # one alignment exactly / none / a few
    Case("tight", "tight", 9, (_u(600, 0), _u(600, -1), _u(600, 1)), 31),
    # alphabet sizes: no skip transition at all; then the softmax paths (tile kernel with one row per workgroup, its last size, lane per row)
    Case("alphabet-2", "alphabet", 2, (_u(40, 2),), 41),
    Case("alphabet-5088", "alphabet", 5088, (_u(0, T=5), _u(1, T=5), _u(1, T=5)), 42),
    Case("alphabet-10175", "alphabet", 10175, (_u(0, T=5), _u(1, T=5), _u(1, T=5)), 43),
    Case("alphabet-10176", "alphabet", 10176, (_u(0, T=5), _u(1, T=5), _u(1, T=5)), 44),
    # utterances without a frame beside one that has four
    Case("empty", "empty", 6, (_u(1, T=0), _u(2, T=4), _u(3, T=0)), 51),
]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]

Inputs = collections.namedtuple("Inputs", "case A mb maxT acts labels in_len paths feasible")


def repeats_of(lab):
    return sum(int(a == b) for a, b in zip(lab, lab[1:]))


def alignment(lab, T):
    """the labels, a blank between repeated labels, blanks up to T (cut at T where the utterance has no alignment)"""
    path = []
    for i, v in enumerate(lab):
        if i and lab[i - 1] == v:
            path.append(0)
        path.append(int(v))
    path += [0] * max(0, T - len(path))
    return path[:max(T, 0)]


def build(case, peak=PEAK):
    """seeded inputs of a case: acts float32 [maxT * mb, A] in (t, n) row order"""
    rng = np.random.default_rng(case.seed)
    A, mb = case.A, len(case.utts)
    labels, in_len = [], []
    for u in case.utts:
        lab = [int(v) for v in rng.integers(1, A, u.L)]
        if u.L >= 3 and A > 2:   # at least one repeat, and two in a row
            lab[u.L // 2] = lab[u.L // 2 - 1]
            if u.L >= 8:
                lab[u.L // 4 + 1] = lab[u.L // 4] = lab[u.L // 4 - 1]
        labels.append(lab)
        in_len.append(u.T if u.T is not None else u.L + repeats_of(lab) + u.slack)
    in_len = np.array(in_len, np.int32)
    maxT = max(1, int(in_len.max()))
    acts = rng.standard_normal((maxT, mb, A)).astype(np.float32)
    paths = []
    for n, lab in enumerate(labels):
        path = alignment(lab, int(in_len[n]))
        paths.append(path)
        if path:
            acts[np.arange(len(path)), n, path] += np.float32(peak)
    feasible = np.array([t > 0 and len(l) + repeats_of(l) <= t for l, t in zip(labels, in_len)])
    return Inputs(case, A, mb, maxT, acts.reshape(maxT * mb, A), labels, in_len, paths, feasible)


def custom(name, A, utts, seed):
    """inputs of a case outside the list (the limits of the entry points), built the same way"""
    return build(Case(name, "custom", A, tuple(utts), seed))


def flat_labels(inp):
    flat = np.array([v for l in inp.labels for v in l] or [0], np.int32)
    return flat, np.array([len(l) for l in inp.labels], np.int32)


def lattice_shape(inp):
    """(threads per workgroup, sorted slot counts of the feasible utterances) that ctc_lattice_kernel takes for this minibatch: threads
    doubles from 64 up to 512 until it covers the longest S; an utterance uses ceil(S / threads) of the LAT_SLOTS slots per thread"""
    maxS = 2 * max(len(l) for l in inp.labels) + 1
    threads = 64
    while threads < maxS and threads < 512:
        threads *= 2
    slots = sorted({-(-(2 * len(l) + 1) // threads) for l, f in zip(inp.labels, inp.feasible) if f})
    return threads, slots


def log_softmax(x):
    x = np.asarray(x, np.float64)
    z = x - x.max(-1, keepdims=True)
    e = np.exp(z)
    return np.where(e == 0, -np.inf, z - np.log(e.sum(-1, keepdims=True)))   # a probability that underflows is zero: log p = -inf


def _skips(lwb):
    """may state s be entered from s - 2: it is a label, and not the label two states back"""
    skip = np.zeros(len(lwb), bool)
    skip[2:] = (lwb[2:] != 0) & (lwb[2:] != lwb[:-2])
    return skip


def _lattice(lp, skip):
    """alpha [T, S] for emission terms lp [T, S] (beta: the same recursion on the mirrored problem); the only Python loop is over frames"""
    T, S = lp.shape
    out = np.full((T, S), -np.inf)
    out[0, :2] = lp[0, :2]
    one = np.full(S, -np.inf)
    two = np.full(S, -np.inf)
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            prev = out[t - 1]
            one[1:] = prev[:-1]
            two[2:] = np.where(skip[2:], prev[:-2], -np.inf)
            np.logaddexp(prev, one, out=out[t])
            np.logaddexp(out[t], two, out=out[t])
            out[t] += lp[t]
    return out


def _utterance(logp, lab, T, A):
    """-> (cost, grad [T, A]) of one feasible utterance from its log-probabilities logp [T, A]"""
    L = len(lab)
    S = 2 * L + 1
    lwb = np.zeros(S, np.int64)
    lwb[1::2] = lab
    lp = logp[:, lwb]                                                # [T, S]
    alpha = _lattice(lp, _skips(lwb))
    # beta is alpha of the mirrored problem: frames and states reversed, so that the skip out of s into s + 2 becomes one into s' from s' - 2
    beta = _lattice(lp[::-1, ::-1], _skips(lwb[::-1]))[::-1, ::-1]
    logZ = np.logaddexp(alpha[T - 1, S - 1], alpha[T - 1, S - 2]) if S > 1 else alpha[T - 1, 0]
    ab = alpha + beta                                                # both include the emission of their frame, as in the reference
    order = np.argsort(lwb, kind="stable")
    present, first = np.unique(lwb[order], return_index=True)
    with np.errstate(invalid="ignore"):
        red = np.logaddexp.reduceat(ab[:, order], first, axis=1)     # [T, labels present]
    out = np.full((T, A), -np.inf)
    out[:, present] = red
    p = np.exp(logp)
    with np.errstate(invalid="ignore", over="ignore"):
        grad = p - np.exp(out - logp - logZ)
    grad = np.where(np.isneginf(out), p, grad)
    return -logZ, grad


def reference(acts, labels, in_len, probs=False):
    labels = [list(l) for l in labels]
    mb = len(labels)
    acts = np.asarray(acts)
    A = acts.shape[-1]
    maxT = acts.size // (mb * A)
    x = acts.reshape(maxT, mb, A).astype(np.float64)
    costs = np.zeros(mb)
    grads = np.zeros((maxT, mb, A))
    for n, lab in enumerate(labels):
        T = int(in_len[n])
        if T <= 0 or len(lab) + repeats_of(lab) > T:
            continue
        with np.errstate(divide="ignore"):
            logp = np.log(x[:T, n]) if probs else log_softmax(x[:T, n])
        costs[n], grads[:T, n] = _utterance(logp, lab, T, A)
    return costs, grads


def closed_form_cost(acts, n, mb, path):
    acts = np.asarray(acts)
    A = acts.shape[-1]
    x = acts.reshape(-1, mb, A)[:len(path), n]
    return float(-log_softmax(x)[np.arange(len(path)), path].sum())


def distances(inp, costs, grads, costs64, grads64):
    """per utterance: (relative cost distance, relative l2 distance of the rows t < T, largest element difference there)"""
    g = np.asarray(grads, np.float64).reshape(inp.maxT, inp.mb, inp.A)
    out = []
    for n in range(inp.mb):
        T = int(inp.in_len[n]) if inp.feasible[n] else 0
        dc = abs(float(costs[n]) - costs64[n]) / max(abs(costs64[n]), 1e-30) if costs64[n] != 0 else abs(float(costs[n]))
        d = g[:T, n] - grads64[:T, n]
        den = np.linalg.norm(grads64[:T, n])
        out.append((dc, float(np.linalg.norm(d) / den) if den > 0 else float(np.linalg.norm(d)), float(np.abs(d).max()) if d.size else 0.0))
    return out


def bars(d_ref, margin=MARGIN):
    """the (cost, l2, element) distances to float64 allowed on an utterance whose oracle distances are d_ref"""
    return max(margin * d_ref[0], FLOOR_COST), max(margin * d_ref[1], FLOOR_L2), max(margin * d_ref[2], FLOOR_EL)


def ratios(d, d_ref):
    """distance over the oracle's distance, the oracle's taken no smaller than a quarter of the floor (below it fp32 is simply accurate and
    the quotient of two roundings says nothing): a ratio <= MARGIN is inside the bar"""
    return tuple(a / max(b, f / 4.0) for a, b, f in zip(d, d_ref, (FLOOR_COST, FLOOR_L2, FLOOR_EL)))
