"""CPU-only: pins the float64 CTC model of tests/ctc_ref.py, which tests/test_ctc_edges_gpu.py holds the HIP kernels to, and measures how
far the oracle's fp32 restatement of the reference (oracle/aslp_oracle_ctc.c) lies from it on the cases of that file.

(a) The model reproduces what the REFERENCE's own CPU code produced (tests/golden/ctc_*.bin): costs within 1e-5 relative, gradients within
    1e-4 relative l2 (the fixtures are short: fp32 is accurate there), the same infinite costs, exact zeros where the fixtures have zeros.
(b) Where exactly one alignment exists (the tight case, slack 0) the cost is -sum_t log p_t(path_t): the model's lattice gives it to 1e-12.
(c) d_ref, the oracle's distance to the model, for every utterance of every case: printed, and held below 5e-3 (gradient, relative l2) and
    5e-6 (cost, relative).  The GPU bar is MARGIN x d_ref per utterance; it means something only while d_ref itself is small."""
import numpy as np
import pytest

import ctc_golden
import ctc_ref as ref
from test_oracle_ctc_cpu import orc_ctc

_cache = {}


def case_data(oracle, name):
    """inputs, the float64 result and the oracle's result of a case: computed once per process, shared, never modified"""
    if name not in _cache:
        inp = ref.build(ref.BY_NAME[name])
        c64, g64 = ref.reference(inp.acts, inp.labels, inp.in_len)
        flat, lab_len = ref.flat_labels(inp)
        oc, og = orc_ctc(oracle, inp.acts.reshape(-1).copy(), flat, lab_len, inp.in_len, inp.A, inp.mb)
        _cache[name] = (inp, c64, g64, oc, og.reshape(inp.maxT, inp.mb, inp.A))
    return _cache[name]


@pytest.mark.parametrize("name", ctc_golden.CASES)
def test_model_reproduces_reference_fixtures(name):
    g = ctc_golden.load(name)
    A, mb, maxT = g["A"], g["mb"], g["maxT"]
    labels, o = [], 0
    for l in g["label_lengths"]:
        labels.append([int(v) for v in g["flat_labels"][o:o + l]])
        o += l
    costs, grads = ref.reference(g["acts"].reshape(maxT * mb, A), labels, g["input_lengths"])
    assert np.array_equal(np.isinf(costs), np.isinf(g["costs"])) and not np.isnan(costs).any()
    fin = np.isfinite(g["costs"])
    rel = np.abs(costs[fin] - g["costs"][fin]) / np.maximum(np.abs(g["costs"][fin]), 1e-30)
    assert (rel[g["costs"][fin] != 0] <= 1e-5).all() and (costs[fin][g["costs"][fin] == 0] == 0).all(), rel
    gr, want = grads.reshape(-1), g["grads"].astype(np.float64)
    assert not np.isnan(gr).any()
    assert np.linalg.norm(gr - want) <= 1e-4 * np.linalg.norm(want)
    assert (gr[want == 0] == 0).all()


def test_single_alignment_cost_is_the_closed_form():
    inp = ref.build(ref.BY_NAME["tight"])
    assert list(inp.feasible) == [True, False, True]
    lab = inp.labels[0]
    assert len(lab) + ref.repeats_of(lab) == inp.in_len[0] == len(inp.paths[0])     # exactly one alignment, and it is the favoured one
    costs, grads = ref.reference(inp.acts, inp.labels, inp.in_len)
    closed = ref.closed_form_cost(inp.acts, 0, inp.mb, inp.paths[0])
    assert abs(costs[0] - closed) <= 1e-12 * abs(closed)
    g = grads.reshape(inp.maxT, inp.mb, inp.A)
    assert costs[1] == 0 and (g[:, 1] == 0).all()                                  # one frame short: no alignment
    # with one alignment the posterior of every frame is the path's label: grad = p - onehot(path)
    p = np.exp(ref.log_softmax(inp.acts.reshape(inp.maxT, inp.mb, inp.A)[:inp.in_len[0], 0]))
    p[np.arange(len(inp.paths[0])), inp.paths[0]] -= 1.0
    assert np.abs(g[:inp.in_len[0], 0] - p).max() <= 1e-9


def test_case_list_reaches_every_rung_and_slot_count():
    """computed from maxS and S as csrc/ctc.hip does: 64, 128, 256, 512 threads, 1..8 slots, and the shapes the issue of the softmax names"""
    seen = {}
    for c in ref.CASES:
        threads, slots = ref.lattice_shape(ref.build(c))
        seen.setdefault(threads, set()).update(slots)
    assert sorted(seen) == [64, 128, 256, 512] and seen[512] == set(range(1, ref.LAT_SLOTS + 1)), seen
    S = sorted({2 * u.L + 1 for c in ref.CASES for u in c.utts})
    for edge in (63, 65, 127, 129, 255, 257, 511, 513, 4095):
        assert edge in S, edge
    for A, rows in ((5088, 1), (10175, 1), (10176, 0)):   # rows of a 40 KB tile (pitch A | 1); 0: the lane-per-row kernel
        assert A in [c.A for c in ref.CASES] and min(64, (40 * 1024 // 4 - 64) // (A | 1)) == rows
    assert min(64, (40 * 1024 // 4 - 64) // (5087 | 1)) == 2


def test_oracle_distance_to_model(oracle):
    """d_ref per utterance; the caps keep the derived GPU bar meaningful"""
    worst_l2 = worst_cost = 0.0
    print("\nd_ref: oracle (fp32) against the float64 model, per utterance")
    print("%-16s %5s %6s %9s %9s %9s" % ("case", "L", "T", "cost", "grad l2", "grad max"))
    for name in ref.NAMES:
        inp, c64, g64, oc, og = case_data(oracle, name)
        assert not np.isnan(og).any() and not np.isnan(g64).any()
        for n, (dc, l2, el) in enumerate(ref.distances(inp, oc, og, c64, g64)):
            print("%-16s %5d %6d %9.2e %9.2e %9.2e%s" % (name, len(inp.labels[n]), inp.in_len[n], dc, l2, el, "" if inp.feasible[n] else "  (no alignment)"))
            worst_l2, worst_cost = max(worst_l2, l2), max(worst_cost, dc)
            if not inp.feasible[n]:
                assert oc[n] == 0 and c64[n] == 0 and (og[:, n] == 0).all() and (g64[:, n] == 0).all()
            assert (og[inp.in_len[n]:, n] == 0).all() and (g64[inp.in_len[n]:, n] == 0).all()
    print("worst: cost %.2e (cap %.0e), gradient %.2e (cap %.0e)" % (worst_cost, ref.CAP_REF_COST, worst_l2, ref.CAP_REF_L2))
    assert worst_l2 <= ref.CAP_REF_L2 and worst_cost <= ref.CAP_REF_COST
