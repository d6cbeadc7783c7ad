"""Pins tests/ctc_errors_ref.py, the model the GPU tests of the device token-error path compare with: against the oracle's
orc_ctc_token_errors on random ragged batches and against hand-computed cases."""
import ctypes as C

import numpy as np
import pytest

import ctc_errors_ref as ref

i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")


def orc_token_errors(oracle, seq, label):
    fn = oracle.lib.orc_ctc_token_errors
    fn.restype = C.c_int
    fn.argtypes = [f32p, C.c_int, C.c_int, C.c_int, i32p, C.c_int, C.POINTER(C.c_int)]
    hl = C.c_int()
    seq = np.ascontiguousarray(seq, np.float32)
    lab = np.array(list(label) or [0], np.int32)
    return fn(seq, seq.shape[1], seq.shape[0], seq.shape[1], lab, len(label), C.byref(hl)), hl.value


@pytest.mark.parametrize("A,mb,maxT,seed", [(5, 4, 12, 0), (29, 7, 40, 1), (128, 3, 90, 2), (3, 9, 33, 3)])
def test_model_matches_oracle_on_ragged_batches(oracle, A, mb, maxT, seed):
    rng = np.random.default_rng(seed)
    for trial in range(4):
        in_len = rng.integers(1, maxT + 1, mb).astype(np.int32)
        in_len[trial % mb] = maxT
        labels = [[int(v) for v in rng.integers(1, A, int(rng.integers(0, maxT)))] for _ in range(mb)]
        acts = rng.standard_normal((maxT * mb, A)).astype(np.float32)
        # a sharper batch too: long runs of one id, so that collapsing does something
        if trial % 2:
            acts = np.repeat(acts.reshape(maxT, mb, A)[::3], 3, axis=0)[:maxT].reshape(maxT * mb, A).copy()
        errors, hyps = ref.token_errors(acts, labels, in_len)
        for s in range(mb):
            seq = acts.reshape(maxT, mb, A)[:in_len[s], s]
            want, hyp_len = orc_token_errors(oracle, seq, labels[s])
            assert errors[s] == want and len(hyps[s]) == hyp_len, (trial, s)


def test_argmax_earliest_column_wins(oracle):
    m = np.array([[0.5, 0.5, 0.1], [0.1, 0.7, 0.7], [-3.0, -3.0, -3.0], [1.0, 2.0, 3.0]], np.float32)
    assert ref.argmax_first(m).tolist() == [0, 1, 0, 2]
    rng = np.random.default_rng(5)
    x = rng.integers(-2, 3, (200, 17)).astype(np.float32)   # many ties
    assert np.array_equal(ref.argmax_first(x), oracle.find_row_max_id(x))
    assert ref.argmax_first(np.full((1, 4), np.nan, np.float32)).tolist() == [-1]


def test_collapse_by_hand():
    assert ref.collapse([0, 1, 1, 0, 2, 2, 2, 0, 0, 3]) == [1, 2, 3]
    assert ref.collapse([0, 0, 0]) == []
    assert ref.collapse([4]) == [4]
    assert ref.collapse([0]) == []
    assert ref.collapse([7] * 9) == [7]
    assert ref.collapse([2, 0, 2]) == [2, 2]
    assert ref.collapse([2, 2]) == [2]
    assert ref.collapse([1, 2, 1, 2]) == [1, 2, 1, 2]
    assert ref.collapse([]) == []


def test_edit_distance_by_hand():
    ed = ref.edit_distance
    assert ed([1, 2, 3], [1, 2, 3]) == 0
    assert ed([1, 3], [1, 2, 3]) == 1
    assert ed([2, 2, 2, 2], [1, 2, 3]) == 3
    assert ed([], [1, 2, 3]) == 3
    assert ed([1, 2, 3], []) == 3
    assert ed([], []) == 0
    assert ed([1, 1], [1]) == 1
    # kitten / sitting as numbers: 3
    assert ed([11, 9, 20, 20, 5, 14], [19, 9, 20, 20, 9, 14, 7]) == 3
    # disjoint alphabets: max(H, R)
    assert ed([1] * 5, [2] * 8) == 8 and ed([1] * 8, [2] * 5) == 8
    # a shift by one costs two (one deletion, one insertion), not len
    assert ed(list(range(1, 11)), list(range(2, 12))) == 2


def test_edit_distance_scan_form_matches_textbook_loop():
    rng = np.random.default_rng(11)
    for trial in range(200):
        R, H = int(rng.integers(0, 14)), int(rng.integers(0, 14))
        a = rng.integers(1, 4, R).tolist()
        b = rng.integers(1, 4, H).tolist()
        assert ref.edit_distance(a, b) == ref.edit_distance_textbook(a, b), (a, b)


def test_token_errors_layout_by_hand():
    # three interleaved utterances of 5 / 3 / 4 frames, rows t * 3 + s; rows past an utterance's end are poison
    paths = [[1, 1, 0, 1, 2], [0, 3, 3], [2, 0, 0, 2]]
    A, mb, maxT = 5, 3, 5
    acts = np.full((maxT * mb, A), np.nan, np.float32)
    for s, p in enumerate(paths):
        acts.reshape(maxT, mb, A)[:len(p), s] = ref.one_hot(p, A)
    errors, hyps = ref.token_errors(acts, [[1, 1, 2], [4], []], [5, 3, 4])
    assert hyps == [[1, 1, 2], [3], [2, 2]]
    assert errors.tolist() == [0, 1, 2]
    errors, hyps = ref.token_errors(ref.one_hot([0, 2, 2, 0, 2], 3), [[2]])
    assert hyps == [[2, 2]] and errors.tolist() == [1]


def test_path_for_builds_the_asked_hypothesis():
    rng = np.random.default_rng(2)
    for hyp, T in (([], 4), ([3], 1), ([3, 3], 3), ([1, 2, 2, 1], 11), ([5] * 6, 11)):
        ids = ref.path_for(hyp, T, rng)
        assert len(ids) == T and ref.collapse(ids) == hyp
