"""A plain numpy model of the CTC token errors (WarpCtc::ErrorRate, warp-ctc.cc:487-529; Ctc::ErrorRate / ErrorRateMSeq,
ctc-loss.cc:346-424): row argmax with the earliest column winning (cu-matrix.cc:1493-1510), best path = repeats collapsed then blanks
dropped, textbook unit-cost edit distance.  Pinned against the oracle and hand-computed cases in test_ctc_errors_ref_cpu.py; the GPU
tests compare the device path with it, demanding equality."""
import numpy as np

BLANK = 0


def argmax_first(m):
    """id of the first strict maximum of every row, starting from -1e21; -1 where no element beats it (a row of NaN)"""
    m = np.asarray(m, np.float32)
    ids = np.full(m.shape[0], -1, np.int32)
    best = np.full(m.shape[0], np.float32(-1e21), np.float32)
    for c in range(m.shape[1]):
        with np.errstate(invalid="ignore"):
            better = best < m[:, c]
        ids[better] = c
        best[better] = m[better, c]
    return ids


def collapse(ids):
    """frame f emits its id iff id != blank and (f == 0 or id != id(f - 1))"""
    hyp, prev = [], None
    for f, i in enumerate(ids):
        i = int(i)
        if (f == 0 or i != prev) and i != BLANK:
            hyp.append(i)
        prev = i
    return hyp


def edit_distance(ref, hyp):
    """d[h][r] = min(d[h-1][r] + 1, d[h][r-1] + 1, d[h-1][r-1] + (hyp[h-1] != ref[r-1])), one vectorised row at a time: the running
    minimum over r of (min(up + 1, diagonal + diff) - r) carries the left neighbour's + 1"""
    ref = np.asarray(ref, np.int64).reshape(-1)
    R = ref.size
    prev = np.arange(R + 1, dtype=np.int64)
    ramp = np.arange(R + 1, dtype=np.int64)
    for h, tok in enumerate(hyp, 1):
        cand = np.empty(R + 1, np.int64)
        cand[0] = h
        cand[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (ref != tok))
        prev = np.minimum.accumulate(cand - ramp) + ramp
    return int(prev[R])


def edit_distance_textbook(ref, hyp):
    """the quadratic double loop, for small cases: what edit_distance is checked against"""
    R, H = len(ref), len(hyp)
    d = [[0] * (R + 1) for _ in range(H + 1)]
    for r in range(R + 1):
        d[0][r] = r
    for h in range(1, H + 1):
        d[h][0] = h
        for r in range(1, R + 1):
            d[h][r] = min(d[h - 1][r] + 1, d[h][r - 1] + 1, d[h - 1][r - 1] + (hyp[h - 1] != ref[r - 1]))
    return d[H][R]


def token_errors(acts, labels, input_lengths=None):
    """acts [(maxT * mb) x A], row t * mb + n; input_lengths None: one sequence of all rows.  Returns (errors int32[mb], hyps)."""
    acts = np.asarray(acts, np.float32)
    mb = len(labels)
    if input_lengths is None:
        assert mb == 1
        input_lengths = [acts.shape[0]]
    errors, hyps = np.zeros(mb, np.int32), []
    for n in range(mb):
        T = int(input_lengths[n])
        rows = acts[n:n + (T - 1) * mb + 1:mb] if T > 0 else acts[:0]
        hyp = collapse(argmax_first(rows))
        hyps.append(hyp)
        errors[n] = edit_distance(labels[n], hyp)
    return errors, hyps


def one_hot(ids, A, dtype=np.float32):
    """activations whose argmax path is `ids`"""
    ids = np.asarray(ids, np.int64)
    m = np.zeros((ids.size, A), dtype)
    m[np.arange(ids.size), ids] = 1.0
    return m


def path_for(hyp, T, rng=None):
    """a frame id sequence of length T whose best path is `hyp` (tokens != 0): a blank between equal neighbours, the rest of the frames
    filled with repeats and blanks"""
    ids = []
    for k, tok in enumerate(hyp):
        if k > 0 and hyp[k - 1] == tok:
            ids.append(BLANK)
        ids.append(int(tok))
    assert len(ids) <= T, "T too small for this hypothesis"
    while len(ids) < T:
        at = int(rng.integers(0, len(ids) + 1)) if (rng is not None and ids) else len(ids)
        if at > 0 and ids[at - 1] != BLANK:
            ids.insert(at, ids[at - 1])   # a repeat of the frame before: collapses
        elif at < len(ids) and ids[at] != BLANK:
            ids.insert(at, ids[at])       # a repeat of the frame after
        else:
            ids.insert(at, BLANK)
    assert collapse(ids) == [int(t) for t in hyp]
    return ids
