"""float64 model of MultiTaskLoss over a <BlockSoftmax> output with one label per (row, xent task), and the cases the kernel and engine
tests share: block softmax (nnet-activation.h:64-143), the labelled multitask diff and per-task sums (nnet-loss.cc:63-156, 341-368) and
the component's backward mask (nnet-activation.h:118-131: diff *= 1 - sum of the block's diff row).

A label is a column relative to its block; a label < 0 or >= the block's width is "no target": the row's target is all zeros, its sum 0
switches the frame off in that task (nnet-loss.cc:80-85)."""
import collections

import numpy as np

ARGMAX_GAP = 1e-3

# rows; block widths; block offsets (None: one behind the other); the column of the operands' buffers at which the matrix starts
Case = collections.namedtuple("Case", "name rows widths offsets base")
CASES = [
    Case("wave_slot_edge", 5, [3, 1, 64, 65], None, 0),
    Case("more_blocks_than_waves", 7, [10, 20, 30, 40, 50], None, 0),
    Case("narrow_medium_edge", 3, [512, 513], None, 0),
    Case("medium_aligned", 4, [516, 40], None, 0),
    Case("medium_offset3", 4, [516, 40], None, 3),
    Case("slots8", 2, [1028], None, 0),
    Case("slots16", 2, [2052, 7], None, 0),
    Case("slots32", 1, [8192], None, 0),
    Case("gap", 6, [12, 9], [0, 14], 0),
    Case("grid_stride", 300, [7, 33], None, 0),   # more rows than workgroups: a workgroup's second row, its maximum over two rows
]
CASE_NAMES = [c.name for c in CASES]
FRAME_WEIGHTS = np.array([0.0, 1.0, 2.0], np.float32)
TASK_WEIGHTS = [1.0, 0.25, 0.0]


def offsets_of(case):
    if case.offsets is not None:
        return list(case.offsets)
    return [int(x) for x in np.concatenate([[0], np.cumsum(case.widths)[:-1]])]


def total_cols(case):
    off = offsets_of(case)
    return off[-1] + case.widths[-1]


def softmax(a):
    a = np.asarray(a, np.float64)
    e = np.exp(a - a.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def block_softmax(acts, blocks):
    """blocks: [(offset, cols)]; columns of no block stay as they are"""
    out = np.array(acts, np.float64)
    for off, cols in blocks:
        out[:, off:off + cols] = softmax(out[:, off:off + cols])
    return out


def argmax_gap(p):
    """per row: (largest - second largest) / largest"""
    top = np.partition(np.asarray(p, np.float64), -2, axis=-1)[:, -2:]
    return (top[:, 1] - top[:, 0]) / top[:, 1]


def safe_logits(rng, rows, cols, scale=3.0):
    """logits whose float64 softmax and its fp32 rounding both have a clear arg-max in every row, so that no rounding decides `correct`"""
    logits = (rng.standard_normal((rows, cols)) * scale).astype(np.float32)
    if cols < 2:
        return logits
    for _ in range(100):
        p = softmax(logits)
        bad = np.flatnonzero((argmax_gap(p) <= 2 * ARGMAX_GAP) | (argmax_gap(p.astype(np.float32)) <= 2 * ARGMAX_GAP))
        if bad.size == 0:
            return logits
        logits[bad] = (rng.standard_normal((bad.size, cols)) * scale).astype(np.float32)
    raise AssertionError("no clear arg-max after 100 draws")


def inputs(case):
    """activations [rows x total_cols] (NaN in the columns of no block), labels [rows x blocks] int32, frame weights, task weights"""
    k = CASE_NAMES.index(case.name)
    rng = np.random.default_rng(9100 + k)
    rows, off = case.rows, offsets_of(case)
    acts = np.full((rows, total_cols(case)), np.nan, np.float32)
    labels = np.empty((rows, len(case.widths)), np.int32)
    for b, (o, c) in enumerate(zip(off, case.widths)):
        acts[:, o:o + c] = safe_logits(rng, rows, c)
        labels[:, b] = rng.integers(0, c, rows)
        labels[2::3, b] = softmax(acts[:, o:o + c]).argmax(1)[2::3]   # every third row is classified correctly
        if rows >= 4:
            labels[(b + 1) % rows, b] = -1                            # no target
            labels[(b + 3) % rows, b] = c + (b % 2) * 1000            # at or beyond the block's width: no target either
        elif rows >= 2 and b == 0:                                    # (few rows: one of them, in one block, so that live rows remain)
            labels[1, b] = -1 if k % 2 else c
    fw = FRAME_WEIGHTS[(np.arange(rows) + k) % 3].copy() if rows >= 4 else FRAME_WEIGHTS[[2, 1, 0][:rows]].copy()
    weights = [TASK_WEIGHTS[(b + k) % 3] for b in range(len(case.widths))]
    return acts, labels, fw, weights


def model(post, blocks, weights, labels, fw, mask):
    """post: the posteriors (any float type) [rows x >= all blocks].  Returns the float64 diff (zeros in the columns of no block) and per
    block dict(frames, correct, loss, entropy, likelyhood): the increments Xent's accumulators take (nnet-loss.cc:107-131)."""
    post = np.asarray(post, np.float64)
    rows = post.shape[0]
    fw = np.asarray(fw, np.float64)
    diff = np.zeros_like(post)
    stats = []
    for b, ((off, cols), wt) in enumerate(zip(blocks, weights)):
        y = post[:, off:off + cols]
        lab = np.asarray(labels)[:, b]
        has = (lab >= 0) & (lab < cols)
        t = np.zeros((rows, cols))
        t[np.flatnonzero(has), lab[has]] = 1.0
        wr = fw * has
        d = (y - t) * wr[:, None] * np.float64(np.float32(wt))
        if mask:
            d = d * (1.0 - d.sum(axis=1, keepdims=True))
        diff[:, off:off + cols] = d
        y_lab = np.where(has, y[np.arange(rows), np.where(has, lab, 0)], 1.0)
        stats.append(dict(frames=float(wr.sum()), correct=float((wr * (y.argmax(1) == np.where(has, lab, 0))).sum()),
                          loss=float(-(wr * np.log(y_lab + 1e-20)).sum()), entropy=float(-(wr * np.log(1.0 + 1e-20)).sum()),
                          likelyhood=float((wr * np.where(has, y_lab, 0.0)).sum())))
    return diff, stats


def dense_targets(case_or_blocks, labels, total):
    """the labels as MultiTaskLoss' dense target matrix: one-hot rows, a zero row where there is no target"""
    blocks = case_or_blocks
    t = np.zeros((np.asarray(labels).shape[0], total), np.float32)
    for b, (off, cols) in enumerate(blocks):
        lab = np.asarray(labels)[:, b]
        has = (lab >= 0) & (lab < cols)
        t[np.flatnonzero(has), off + lab[has]] = 1.0
    return t


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    den = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / den) if den > 0 else float(np.linalg.norm(a - b))
