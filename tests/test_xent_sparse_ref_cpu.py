"""The CSR rules of Xent's sparse-target path as a model (tests/xent_sparse_ref.py), checked on the CPU: csr -> dense equals a direct
restatement of PosteriorToMatrix on random posteriors with duplicates, negative pdfs and empty frames; the adversarial rows the GPU
tests hand to the kernel have the property they are named for; every kind is met at every slots-per-thread rung."""
import numpy as np
import pytest

import bn_xent_ref as ref
import xent_sparse_ref as sp


def random_posterior(rng, frames, num_cols):
    post = []
    for _ in range(frames):
        n = int(rng.choice([0, 1, 1, 2, 3, 5]))
        frame = [(int(rng.integers(-2, 0) if rng.random() < 0.15 else rng.integers(0, num_cols)), np.float32(rng.uniform(-1, 1)))
                 for _ in range(n)]
        if n >= 2 and rng.random() < 0.5:
            frame.append((frame[0][0], np.float32(rng.uniform(0, 1))))     # a duplicate: the later one wins
        post.append(frame)
    return post


@pytest.mark.parametrize("num_cols", [1, 7, 40, 3000])
def test_csr_round_trip_is_posterior_to_matrix(num_cols):
    rng = np.random.default_rng(num_cols)
    post = random_posterior(rng, 64, num_cols)
    assert any(len(f) == 0 for f in post) and any(c < 0 for f in post for c, _ in f)
    assert any(len({c for c, _ in f}) < len(f) for f in post)
    rb, cols, w = sp.posterior_to_csr(post, num_cols)
    assert sp.csr_is_valid(rb, cols, len(post)) and (cols >= 0).all() and (cols < num_cols).all()
    dense, direct = sp.csr_to_dense(rb, cols, w, num_cols), sp.posterior_to_matrix(post, num_cols)
    assert np.array_equal(dense.view(np.int32), direct.view(np.int32))


def test_later_duplicate_wins_and_out_of_bound_is_an_error():
    rb, cols, w = sp.posterior_to_csr([[(3, 0.25), (1, 0.5), (3, 0.75)], [], [(-1, 1.0)]], 4)
    assert rb.tolist() == [0, 2, 2, 2] and cols.tolist() == [1, 3] and w.tolist() == [0.5, 0.75]
    for fn in (sp.posterior_to_csr, sp.posterior_to_matrix):
        with pytest.raises(ValueError, match="Out-of-bound Posterior element with index 4, higher than number of columns 4"):
            fn([[(4, 1.0)]], 4)


def test_dense_value_is_zero_plus_weight():
    m = sp.csr_to_dense(np.array([0, 2], np.int32), np.array([0, 2], np.int32), np.array([-0.0, -0.5], np.float32), 3)
    assert not np.signbit(m[0, 0]) and m[0, 2] == -0.5


@pytest.mark.parametrize("name", sp.SPARSE_NAMES)
def test_adversarial_rows_have_their_property(name):
    case = ref.XENT_BY_NAME[name]
    t = sp.sparse_targets(case)
    cols = case.cols
    assert sp.csr_is_valid(t.row_begin, t.cols, case.rows)
    inp = ref.xent_inputs(case)
    untouched = [r for r in range(case.rows) if r not in t.kinds]
    assert np.array_equal(t.dense[untouched], inp.soft[untouched]) and np.array_equal(t.fw[untouched], inp.fw[untouched])
    for r, kind in t.kinds.items():
        c, w = t.cols[t.row_begin[r]:t.row_begin[r + 1]], t.weights[t.row_begin[r]:t.row_begin[r + 1]]
        d = t.dense[r]
        inside = (c >= 0) & (c < cols)
        assert np.count_nonzero(d) <= inside.sum()
        if kind == "empty":
            assert len(c) == 0 and not d.any()
        elif kind == "one":
            assert len(c) == 1 and w[0] == 1.0 and d.sum() == 1.0
        elif kind in ("one-0.3", "fw0"):
            assert len(c) == 1 and w[0] == np.float32(0.3)
        elif kind == "ends":
            assert c.tolist() == ([0, cols - 1] if cols > 1 else [0]) and d[0] != 0 and d[-1] != 0
        elif kind == "sum0":
            assert len(c) == 2 and np.float32(w[0]) + np.float32(w[1]) == 0.0 and d.sum(dtype=np.float32) == 0.0 and np.count_nonzero(d) == 2
        elif kind == "negative":
            assert (w < 0).all() and d.max() == 0.0 and d[int(np.argmax(d))] == 0.0   # arg-max over all columns answers a zero column
        elif kind == "tie":
            top = np.flatnonzero(d == d.max())
            assert len(top) == 2 and d.argmax() == top[0] < top[1]
        elif kind == "negzero":
            assert np.signbit(w).any() and not np.signbit(d).any() and np.count_nonzero(d) == 1
        elif kind == "outside":
            assert c[0] == -1 and c[-1] == cols and inside.sum() == 1 and np.count_nonzero(d) == 1
        elif kind == "dense":
            assert cols <= sp.DENSE_MAX_COLS and len(c) == cols and np.count_nonzero(d) == cols
        assert t.fw[r] == (0.0 if kind == "fw0" else 0.5)
    if case.rows > ref.XENT_MAX_GRID:                                # a workgroup's second row stages other columns than its first
        assert all(ref.XENT_MAX_GRID + j in t.kinds for j in range(4))
        first, second = ref.XENT_MAX_GRID + 1, 1                        # (row 4097 follows row 1 in workgroup 1)
        assert t.kinds[ref.XENT_MAX_GRID] == "empty"
        assert set(t.cols[t.row_begin[first]:t.row_begin[first + 1]]) != set(t.cols[t.row_begin[second]:t.row_begin[second + 1]])


def test_float64_model_on_the_sparse_targets():
    """bn_xent_ref.xent on csr -> dense: a row without targets, with weights summing to 0 or with frame weight 0 counts no frame"""
    case = ref.XENT_BY_NAME["16x1024"]
    inp, t = ref.xent_inputs(case), sp.sparse_targets(case)
    keep = [r for r in range(case.rows) if t.kinds.get(r) not in ("negative", "sum0")]     # (log of a negative target: not a number)
    _, _, sums = ref.xent(inp.post[keep], t.dense[keep], t.fw[keep], False)
    w = t.fw[keep].astype(np.float64) * t.dense[keep].astype(np.float64).sum(1)
    assert np.isfinite(sums).all() and sums[0] == w.sum()
    off = [i for i, r in enumerate(keep) if t.kinds.get(r) in ("empty", "fw0")]
    assert len(off) == 2 and not w[off].any()


def test_every_kind_at_every_rung():
    met = sp.coverage()
    for p in sp.RUNGS:
        assert met[p] == sp.wanted_coverage(p), (p, sorted(sp.wanted_coverage(p) - met[p]))
    assert sp.wanted_coverage(4) == set(sp.KINDS) and sp.wanted_coverage(8) == set(sp.KINDS)
    kernels = {c.kernel for c in sp.SPARSE_CASES}
    assert kernels == {"per%d-%s" % (p, m) for p in sp.RUNGS for m in ("scalar", "vec")}
    # what sparse_targets deals out is what coverage() counts
    got = {p: set() for p in sp.RUNGS}
    for c in sp.SPARSE_CASES:
        if c.rows <= 16:
            got[sp.rung(c.cols)] |= set(sp.sparse_targets(c).kinds.values())
    for p in sp.RUNGS:
        assert got[p] <= met[p] and (got[p] == met[p] or p == 4)
