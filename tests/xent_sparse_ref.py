"""Xent on soft targets given as CSR: the rules as a numpy model, and the targets the GPU tests hand to the kernel.

A posterior is, per frame, a list of (pdf, weight) pairs.  The engine turns it into a dense [frames x pdfs] matrix (PosteriorToMatrix:
a zero matrix, m(t, pdf) = weight by assignment -- a later duplicate wins -- through an add onto the zero; a pdf >= num_cols is an
error, a negative one is dropped) or, since the sparse kernel, into CSR under the same rules: row_begin [frames + 1], the columns sorted
within the frame, the weights.  The kernel's contract is stated on CSR: an entry whose column is outside [0, cols) is skipped, and the
dense value an entry stands for is 0.0f + w.

posterior_to_matrix restates PosteriorToMatrix directly; posterior_to_csr and csr_to_dense are the model of the new path; the round trip
csr -> dense must equal the direct restatement (tests/test_xent_sparse_ref_cpu.py).  sparse_targets(case) gives, for a case of
bn_xent_ref.XENT_CASES, the case's `soft` matrix as CSR with rows overwritten by the adversarial kinds below."""
import collections

import numpy as np

import bn_xent_ref as ref

# the adversarial rows, in the order they are dealt out ("dense" last: it exists only at cols <= DENSE_MAX_COLS)
KINDS = ("empty", "one", "one-0.3", "ends", "sum0", "negative", "tie", "negzero", "outside", "fw0", "dense")
DENSE_MAX_COLS = 1028
RUNGS = (4, 8, 16, 32)
SPARSE_CASES = [c for c in ref.XENT_CASES if c.kernel != "wide"]
SPARSE_NAMES = [c.name for c in SPARSE_CASES]


def rung(cols):
    return next(p for p in RUNGS if -(-cols // 256) <= p)


def posterior_to_matrix(post, num_cols):
    """PosteriorToMatrix: zero matrix, per frame the last weight given for a pdf, added onto the zero"""
    m = np.zeros((len(post), num_cols), np.float32)
    for t, frame in enumerate(post):
        last = {}
        for pdf, w in frame:
            if pdf >= num_cols:
                raise ValueError("Out-of-bound Posterior element with index %d, higher than number of columns %d" % (pdf, num_cols))
            last[int(pdf)] = np.float32(w)
        for pdf, w in last.items():
            if pdf >= 0:                                   # (the scatter skips what lies outside the matrix)
                m[t, pdf] = np.float32(0.0) + w
    return m


def posterior_to_csr(post, num_cols):
    """-> row_begin int32 [frames + 1], cols int32 [nnz], weights float32 [nnz]"""
    row_begin, cols, weights = [0], [], []
    for frame in post:
        last = {}
        for pdf, w in frame:
            if pdf >= num_cols:
                raise ValueError("Out-of-bound Posterior element with index %d, higher than number of columns %d" % (pdf, num_cols))
            if pdf >= 0:
                last[int(pdf)] = np.float32(w)
        for pdf in sorted(last):
            cols.append(pdf)
            weights.append(last[pdf])
        row_begin.append(len(cols))
    return np.array(row_begin, np.int32), np.array(cols, np.int32), np.array(weights, np.float32)


def csr_to_dense(row_begin, cols, weights, num_cols):
    """the dense matrix the kernel's contract names: zeros, m(r, c) = 0.0f + w for the entries with 0 <= c < num_cols"""
    rows = len(row_begin) - 1
    m = np.zeros((rows, num_cols), np.float32)
    for r in range(rows):
        for i in range(row_begin[r], row_begin[r + 1]):
            if 0 <= cols[i] < num_cols:
                m[r, cols[i]] = np.float32(0.0) + np.float32(weights[i])
    return m


def csr_is_valid(row_begin, cols, rows):
    rb = np.asarray(row_begin)
    if len(rb) != rows + 1 or rb[0] != 0 or (np.diff(rb) < 0).any() or rb[-1] != len(cols):
        return False
    return all((np.diff(cols[rb[r]:rb[r + 1]]) > 0).all() for r in range(rows))


def adversarial_row(kind, cols, rng):
    """-> [(column, weight), ...] with strictly increasing columns"""
    f = np.float32
    a, b = sorted(int(v) for v in rng.choice(cols, 2, replace=False)) if cols > 1 else (0, 0)
    if kind == "empty":
        return []
    if kind == "one":
        return [(a, f(1.0))]
    if kind in ("one-0.3", "fw0"):
        return [(a, f(0.3))]
    if kind == "ends":
        return [(0, f(0.25)), (cols - 1, f(0.75))]
    if kind == "sum0":
        return [(a, f(0.5)), (b, f(-0.5))]
    if kind == "negative":
        return [(a, f(-0.25)), (b, f(-0.5))]
    if kind == "tie":                                        # two equal maxima and a smaller third in front of, between or behind them
        c = int(rng.integers(0, cols))
        while c in (a, b):
            c = int(rng.integers(0, cols))
        return sorted([(a, f(0.375)), (b, f(0.375)), (c, f(0.25))])
    if kind == "negzero":
        return [(a, f(-0.0)), (b, f(1.0))]
    if kind == "outside":
        return [(-1, f(0.7)), (a, f(1.0)), (cols, f(0.9))]
    if kind == "dense":
        w = rng.integers(1, 64, cols).astype(np.float32) / np.float32(64 * cols)
        return [(c, w[c]) for c in range(cols)]
    raise KeyError(kind)


SparseTargets = collections.namedtuple("SparseTargets", "case row_begin cols weights fw dense kinds")


def _start(case):
    """where in KINDS a case starts dealing: behind the rows the earlier cases of its rung have used"""
    p = 0
    for c in SPARSE_CASES:
        if c.name == case.name:
            return p
        if rung(c.cols) == rung(case.cols):
            p += min(c.rows, len(KINDS))
    raise KeyError(case.name)


def sparse_targets(case, inp=None):
    """the case's soft targets as CSR, rows 0 .. min(rows, 11) - 1 overwritten by adversarial kinds (dealt out in a cycle that runs on
    through the cases of one slots-per-thread rung; "dense" only at cols <= DENSE_MAX_COLS, elsewhere the row stays); where a workgroup
    takes a second row (rows > XENT_MAX_GRID) rows 4096 .. 4099 get kinds that differ from what rows 0 .. 3 staged.
    kinds: {row: kind}.  fw: the case's frame weights, 0 on the "fw0" rows and 0.5 on the other overwritten rows."""
    inp = inp if inp is not None else ref.xent_inputs(case)
    rng = np.random.default_rng(4000 + ref.XENT_NAMES.index(case.name))
    rows, cols = case.rows, case.cols
    post = [[(int(c), inp.soft[r, c]) for c in np.flatnonzero(inp.soft[r])] for r in range(rows)]
    fw = inp.fw.copy()
    kinds, p = {}, _start(case)
    for j in range(min(rows, len(KINDS))):
        kinds[j] = KINDS[(p + j) % len(KINDS)]
    if rows > ref.XENT_MAX_GRID:
        for j, k in enumerate(("empty", "one-0.3", "ends", "outside")):
            kinds[ref.XENT_MAX_GRID + j] = k
    for r, k in list(kinds.items()):
        if k == "dense" and cols > DENSE_MAX_COLS:
            del kinds[r]
            continue
        post[r] = adversarial_row(k, cols, rng)
        fw[r] = 0.0 if k == "fw0" else 0.5
    row_begin = np.cumsum([0] + [len(f) for f in post]).astype(np.int32)
    ccols = np.array([c for f in post for c, _ in f], np.int32)
    weights = np.array([w for f in post for _, w in f], np.float32)
    return SparseTargets(case, row_begin, ccols, weights, fw, csr_to_dense(row_begin, ccols, weights, cols), kinds)


def coverage():
    """{rung: the kinds met at it over SPARSE_CASES}"""
    met = {p: set() for p in RUNGS}
    for c in SPARSE_CASES:
        p = _start(c)
        for j in range(min(c.rows, len(KINDS))):
            k = KINDS[(p + j) % len(KINDS)]
            if k != "dense" or c.cols <= DENSE_MAX_COLS:
                met[rung(c.cols)].add(k)
    return met


def wanted_coverage(p):
    """every kind at every rung; the fully dense row where the rung has a case of at most DENSE_MAX_COLS columns"""
    has_narrow = any(rung(c.cols) == p and c.cols <= DENSE_MAX_COLS for c in SPARSE_CASES)
    return set(KINDS) - (set() if has_narrow else {"dense"})
