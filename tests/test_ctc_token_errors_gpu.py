"""The device path of the CTC token errors (csrc/ctc_errors.hip: best path + edit distance, one workgroup per utterance behind the row
argmax) against the numpy model of tests/ctc_errors_ref.py, which test_ctc_errors_ref_cpu.py pins to the oracle: errors, hypothesis
lengths and hypotheses must be EQUAL.  Activations are one-hot rows of a chosen id sequence, so H is known by construction; the shapes
are the smallest at which each part of the kernel can go wrong."""
import numpy as np
import pytest
import torch

import ctc_errors_ref as ref

pytestmark = pytest.mark.gpu

# the kernel's own boundaries (csrc/ctc_errors.hip)
HYP_LDS = 2048    # kErrHypLds: hypothesis tokens a workgroup keeps in LDS; a longer one is read back from the scratch slot
MAX_REF = 1024    # kErrMaxRef: one thread per reference token; beyond it the batch takes the host path
WAVE = 64         # the workgroup is the longest reference rounded up to whole waves: R = 64 is one wave, 65 two, 256 four, 257 five


@pytest.fixture(autouse=True)
def device_path(aslp):
    aslp.ops.ctc_errors_on_host(0)
    yield
    aslp.ops.ctc_errors_on_host(-1)


def to_dev(acts, dev, poison=1e9):
    """the matrix as a view of a wider buffer (row stride padded to the next multiple of 16 beyond A), the padding poisoned"""
    acts = np.asarray(acts, np.float32)
    rows, A = acts.shape
    stride = (A // 16 + 1) * 16
    buf = torch.full((rows, stride), poison, dtype=torch.float32, device=dev)
    view = buf[:, :A]
    view.copy_(torch.from_numpy(acts))
    return view


def check(aslp, dev, acts, labels, in_len=None, path=1):
    want_err, want_hyps = ref.token_errors(acts, labels, in_len)
    errors, hyps = aslp.ops.ctc_token_errors(to_dev(acts, dev), labels, in_len)
    assert aslp.lib.aslp_ctc_errors_last_path() == path
    assert [len(h) for h in hyps] == [len(h) for h in want_hyps]
    assert hyps == want_hyps
    assert errors.tolist() == want_err.tolist()
    return errors, hyps


def interleave(seqs, A, poison=np.nan):
    """utterance s owns rows f * num_seq + s; rows past its end hold poison"""
    mb, maxT = len(seqs), max(1, max(len(p) for p in seqs))
    acts = np.full((maxT, mb, A), poison, np.float32)
    for s, p in enumerate(seqs):
        acts[:len(p), s] = ref.one_hot(p, A)
    return acts.reshape(maxT * mb, A), [len(p) for p in seqs]


# ---- collapse ----------------------------------------------------------------------------------------------------------------------
def test_collapse_cases(aslp, dev):
    A = 5
    for path, label, hyp, err in (([0, 0, 0, 0], [1, 2, 3], [], 3),          # all frames blank: H = 0, errors = R
                                  ([1, 1, 0, 2], [], [1, 2], 2),              # R = 0: errors = H
                                  ([3], [3], [3], 0),                         # one frame
                                  ([0], [3], [], 1),                          # one blank frame
                                  ([2] * 9, [2], [2], 0),                     # one token over all frames
                                  ([2, 0, 2], [2, 2], [2, 2], 0),             # a blank a: two tokens
                                  ([2, 2], [2, 2], [2], 1)):                  # a a: one
        errors, hyps = check(aslp, dev, ref.one_hot(path, A), [label])
        assert hyps == [hyp] and errors.tolist() == [err]


def test_argmax_ties(aslp, dev):
    # a tie between column 0 and another: blank wins; between two other columns: the earlier one
    acts = np.array([[0.7, 0.1, 0.7, 0.0], [0.1, 0.7, 0.7, 0.0], [0.1, 0.2, 0.9, 0.9], [0.5, 0.5, 0.5, 0.5]], np.float32)
    errors, hyps = check(aslp, dev, acts, [[1, 2]])
    assert hyps == [[1, 2]] and errors.tolist() == [0]


# ---- layout ------------------------------------------------------------------------------------------------------------------------
def test_interleaved_rows_and_poison_past_the_end(aslp, dev):
    acts, in_len = interleave([[1, 1, 0, 1, 2], [0, 3, 3], [2, 0, 0, 2]], 5)   # A = 5: the stride is padded
    errors, hyps = check(aslp, dev, acts, [[1, 1, 2], [4], []], in_len)
    assert hyps == [[1, 1, 2], [3], [2, 2]] and errors.tolist() == [0, 1, 2]


def test_single_sequence_without_frames(aslp, dev):
    rng = np.random.default_rng(3)
    acts = rng.standard_normal((37, 21)).astype(np.float32)
    check(aslp, dev, acts, [[int(v) for v in rng.integers(1, 21, 9)]], None)


def test_seventy_ragged_utterances(aslp, dev):
    rng = np.random.default_rng(70)
    A, mb = 9, 70
    seqs, labels = [], []
    for s in range(mb):
        T = int(rng.integers(1, 150))
        seqs.append(np.repeat(rng.integers(0, A, T), rng.integers(1, 3, T))[:T].tolist())
        labels.append([int(v) for v in rng.integers(1, A, int(rng.integers(0, 131)))])   # workgroups of one, two and three waves
    acts, in_len = interleave(seqs, A)
    check(aslp, dev, acts, labels, in_len)


def test_random_activations_batch(aslp, dev):
    rng = np.random.default_rng(8)
    A, mb, maxT = 45, 6, 90
    in_len = rng.integers(maxT // 2, maxT + 1, mb)
    in_len[2] = maxT
    acts = rng.standard_normal((maxT * mb, A)).astype(np.float32)
    labels = [[int(v) for v in rng.integers(1, A, int(t) // 3)] for t in in_len]
    check(aslp, dev, acts, labels, in_len)


# ---- distance ----------------------------------------------------------------------------------------------------------------------
def tokens(rng, n, lo=1, hi=6):
    return [int(v) for v in rng.integers(lo, hi, n)]


def test_equal_and_disjoint(aslp, dev):
    rng = np.random.default_rng(1)
    hyp = tokens(rng, 40)
    acts = ref.one_hot(ref.path_for(hyp, 70, rng), 12)
    errors, _ = check(aslp, dev, acts, [hyp])
    assert errors.tolist() == [0]
    for R in (25, 40, 58):   # disjoint alphabets: max(H, R)
        errors, _ = check(aslp, dev, acts, [tokens(rng, R, 7, 12)])
        assert errors.tolist() == [max(40, R)]


@pytest.mark.parametrize("R", [1, WAVE - 1, WAVE, WAVE + 1, 255, 256, 257, MAX_REF - 1, MAX_REF])
def test_reference_lengths_around_the_workgroup_boundaries(aslp, dev, R):
    """one wave / two (63, 64, 65), four / five (255, 256, 257), the served limit; each with H < R, H = R and H > R"""
    assert aslp.lib.aslp_ctc_token_errors_supported(2 * R + 8, R) == 1
    rng = np.random.default_rng(R)
    label = tokens(rng, R)
    seqs = []
    for H in (max(0, R - 7), R, R + 9):
        hyp = label[:H // 2] + tokens(rng, H - H // 2)   # the first half agrees, the rest is a random string over the same tokens
        seqs.append(ref.path_for(hyp, 2 * H + 3, rng))
    acts, in_len = interleave(seqs, 7)
    check(aslp, dev, acts, [label] * 3, in_len)


def test_reference_beyond_the_limit_takes_the_host_path(aslp, dev):
    R = MAX_REF + 1
    assert aslp.lib.aslp_ctc_token_errors_supported(100, R) == 0 and aslp.lib.aslp_ctc_token_errors_supported(100, MAX_REF) == 1
    rng = np.random.default_rng(R)
    label = tokens(rng, R)
    acts, in_len = interleave([ref.path_for(label[:50] + tokens(rng, 30), 100, rng), ref.path_for(tokens(rng, 5), 9, rng)], 7)
    check(aslp, dev, acts, [label, [1, 2]], in_len, path=0)   # one long reference sends the whole batch to the host
    check(aslp, dev, acts, [label[:MAX_REF], [1, 2]], in_len, path=1)


@pytest.mark.parametrize("H", [HYP_LDS - 1, HYP_LDS, HYP_LDS + 1])
def test_hypothesis_around_the_lds_capacity(aslp, dev, H):
    rng = np.random.default_rng(H)
    hyp = tokens(rng, H)
    T = 2 * HYP_LDS   # more frames than the LDS copy holds tokens, so the scratch copy is written in all three cases and read in the last
    label = hyp[100:400] + tokens(rng, 37)
    acts, in_len = interleave([ref.path_for(hyp, T), ref.path_for(tokens(rng, 12), 30, rng)], 7)
    check(aslp, dev, acts, [label, [1]], in_len)


def test_host_switch_gives_the_same_answers(aslp, dev):
    rng = np.random.default_rng(4)
    acts, in_len = interleave([ref.path_for(tokens(rng, 20), 45, rng), ref.path_for(tokens(rng, 31), 50, rng)], 7)
    labels = [tokens(rng, 25), tokens(rng, 25)]
    check(aslp, dev, acts, labels, in_len, path=1)
    aslp.ops.ctc_errors_on_host(1)
    assert aslp.lib.aslp_ctc_errors_on_host_get() == 1
    check(aslp, dev, acts, labels, in_len, path=0)
    aslp.ops.ctc_errors_on_host(0)
    assert aslp.lib.aslp_ctc_errors_on_host_get() == 0
    check(aslp, dev, acts, labels, in_len, path=1)
