"""tests/multitask_ref.py (the float64 model the MultiTaskLoss GPU tests compare with) against the oracle's orc_multitask_eval
(oracle/aslp_oracle.c, the reference's CPU arithmetic restated in C) on the cases the GPU tests use: the labels expanded to one-hot target
rows, a label outside its block to a row of zeros.  The oracle works in fp32, the model in float64: 1e-5 relative."""
import numpy as np
import pytest

import multitask_ref as ref

TOL = 1e-5


@pytest.mark.parametrize("name", ref.CASE_NAMES)
def test_all_xent_model_matches_oracle(oracle, name):
    case = ref.CASES[ref.CASE_NAMES.index(name)]
    acts, labels, fw, weights = ref.inputs(case)
    # the oracle's tasks lie one behind the other: the blocks' windows, without the columns between them
    windows = list(zip(ref.offsets_of(case), case.widths))
    packed = np.concatenate([acts[:, o:o + c] for o, c in windows], axis=1)
    blocks, o = [], 0
    for c in case.widths:
        blocks.append((o, c))
        o += c
    post = ref.block_softmax(packed, blocks).astype(np.float32)
    assert np.isfinite(post).all()
    diff, stats = ref.model(post, blocks, weights, labels, fw, mask=False)
    spec = [("xent", c, w) for c, w in zip(case.widths, weights)]
    want, want_stats = oracle.multitask_eval(spec, fw, post, ref.dense_targets(blocks, labels, o))
    for (off, c), st, wst in zip(blocks, stats, want_stats):
        assert ref.rel_l2(diff[:, off:off + c], want[:, off:off + c]) <= TOL, (name, off)
        assert st["frames"] == wst["frames"] and st["correct"] == wst["correct"], (name, off)
        for k in ("loss", "entropy", "likelyhood"):
            assert abs(st[k] - wst[k]) <= TOL * max(abs(wst[k]), 1e-30) + 1e-12, (name, off, k, st[k], wst[k])


def test_mask_is_block_softmax_backward():
    """nnet-activation.h:118-131 on a diff whose rows do not sum to zero: every row of a block times (1 - its sum)"""
    rng = np.random.default_rng(5)
    post = rng.uniform(0.1, 0.9, (4, 7))
    blocks, labels, fw = [(0, 3), (3, 4)], np.array([[0, 1], [2, -1], [1, 3], [-1, 9]], np.int32), np.array([1.0, 2.0, 0.0, 1.0])
    plain, _ = ref.model(post, blocks, [1.0, 0.5], labels, fw, mask=False)
    masked, _ = ref.model(post, blocks, [1.0, 0.5], labels, fw, mask=True)
    for off, c in blocks:
        d = plain[:, off:off + c]
        assert np.allclose(masked[:, off:off + c], d * (1.0 - d.sum(1, keepdims=True)), rtol=1e-15, atol=0)
    assert (masked[2] == 0).all() and (masked[1, 3:] == 0).all() and (masked[3] == 0).all()   # weight 0 / no target: the row is off
    assert np.abs(masked - plain).max() > 0.05


def test_block_softmax_rows_sum_to_one_per_block():
    rng = np.random.default_rng(6)
    a = rng.standard_normal((5, 9)) * 4
    p = ref.block_softmax(a, [(0, 2), (4, 5)])
    assert np.allclose(p[:, 0:2].sum(1), 1) and np.allclose(p[:, 4:9].sum(1), 1) and np.array_equal(p[:, 2:4], a[:, 2:4])
