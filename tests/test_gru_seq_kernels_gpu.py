"""The 12 persistent GRU kernels of csrc/rnn_persistent.hip (gru_seq_fwd<KW, NP>, gru_seq_bwd<KW1, KW2, NP>: NP = 0 the fp32 instruction, 1 / 2
one / two fp16 pieces per operand; two rungs of H each) against the float64 model of the aslp_gru_seq contract (tests/gru_seq_ref.py, pinned
to the oracle by tests/test_gru_seq_ref_cpu.py, which also counts that the cases below launch all 12).

aslp_gru_seq_forward / _backward are driven through the C ABI on padded buffers (ld = 5H + 8, ldw = K + 4), every case under
aslp_gru_seq_pieces 0, 2 and 1; after every launch the error state, aslp_gru_seq_last_pieces(), and bit for bit everything the launch must not
write (gru_seq_ref.run_on_gpu).  Then tensor by tensor -- z, r, m, g, h and d_z, d_r, d_m, d_g, d_h -- against float64:
  pieces 0 (the fp32 instruction) and 2:  relative l2 error < 1e-5 per tensor, element error < 1e-4 of max(1, largest |reference|)
                                          (lstm_seq_ref.BAR; two pieces must meet the bar of the fp32 instruction: the fp32-equivalence claim)
  pieces 1:                               per case and tensor 2 x d_model (the distance of the one-piece float64 model, CPU) + the bar above,
                                          and not the bits of the two-piece run

Measured on an MI355X, worst over all cases and tensors (relative l2 / element): pieces 0 9.09e-7 / 3.35e-7, pieces 2 8.60e-7 / 3.38e-7 (the
relative l2 worsts belong to H4-S1-T1, whose tensors are 4 numbers each) -- the bar of 1e-5 / 1e-4 stands 11 x above the worst of them, so it is kept as it is (BAR0
below would raise it to 4 x the worst of pieces 0 otherwise); pieces 1 4.02e-4 / 6.30e-4, where the one-piece float64 model alone is
4.03e-4 / 6.30e-4 from the float64 model (MEASURED_WORST below).  The file takes 7 s, 4.6 s of it the two child processes."""
import os
import subprocess
import sys

import ctypes as C
import numpy as np
import pytest
import torch

import gru_seq_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [ref.case_id(c) for c in ref.CASES]
_inputs, _refs, _dmodel, _runs = {}, {}, {}, {}
worst_seen = {}          # pieces -> [l2, element], for the report at the end of the file's run
launch_failed = []       # [(case, pieces, error)]: once a launch ended in an error, nothing further is launched
first_failed_child = []  # once a child ended badly, no further child is started

# worst relative l2 / element error over all cases and tensors on an MI355X, per piece count (printed again by the last test)
MEASURED_WORST = {0: (9.09e-07, 3.35e-07), 2: (8.60e-07, 3.38e-07), 1: (4.02e-04, 6.30e-04)}
# the bar of pieces 0 and 2: the project's, unless it stands less than 4 x above the measured worst of the pieces = 0 kernels
BAR0 = (max(ref.BAR, 4 * MEASURED_WORST[0][0]), max(10 * ref.BAR, 4 * MEASURED_WORST[0][1]))


def inputs(k):
    if k not in _inputs:
        _inputs[k] = ref.build_case(ref.CASES[k])
    return _inputs[k]


def reference(k):
    """the float64 run of case k: computed once, shared, never modified"""
    if k not in _refs:
        _refs[k] = ref.reference(inputs(k))
    return _refs[k]


def d_model(k):
    if k not in _dmodel:
        _dmodel[k] = ref.d_model(inputs(k), reference(k))
    return _dmodel[k]


def guarded(what, fn):
    """fn() unless a launch has failed before; a failure that is not an assertion (the library's error state, the runtime's) bars the rest"""
    if launch_failed:
        pytest.fail("not started: a launch of %s [pieces %s] ended in an error, and nothing more runs on the GPU behind it\n%s" % launch_failed[0])
    try:
        return fn()
    except AssertionError:
        raise
    except Exception as e:
        launch_failed.append(what + (repr(e),))
        raise


def gpu_run(aslp, dev, k, pieces):
    if (k, pieces) not in _runs:
        _runs[(k, pieces)] = guarded((IDS[k], pieces), lambda: ref.run_on_gpu(aslp, torch, dev, inputs(k), pieces, pieces))
    return _runs[(k, pieces)]


def bars_one_piece(k):
    return {name: (2 * l2 + BAR0[0], 2 * el + BAR0[1]) for name, (l2, el) in d_model(k).items()}


def note(pieces, dist):
    w = worst_seen.setdefault(pieces, [0.0, 0.0])
    for l2, el in dist.values():
        w[0], w[1] = max(w[0], l2), max(w[1], el)


@pytest.mark.parametrize("pieces", ref.PIECES)
@pytest.mark.parametrize("k", range(len(ref.CASES)), ids=IDS)
def test_kernels_match_float64_model(aslp, dev, k, pieces):
    got = gpu_run(aslp, dev, k, pieces)
    ry, rd = reference(k)
    dist = ref.distances(ref.CASES[k], got["y"], got["d"], ry, rd)
    note(pieces, dist)
    print("gru-seq %s [pieces %d]: worst relative l2 %.2e, element %.2e" % (IDS[k], pieces, max(v[0] for v in dist.values()), max(v[1] for v in dist.values())))
    ref.compare(inputs(k), got, ry, rd, bars_one_piece(k) if pieces == 1 else BAR0)
    if pieces == 1:   # (every case holds a recurrent product in both passes: tests/test_gru_seq_ref_cpu.py)
        two = gpu_run(aslp, dev, k, 2)
        assert not np.array_equal(got["y"], two["y"]) and not np.array_equal(got["d"], two["d"]), (IDS[k], "one piece gave the two-piece bits")


@pytest.mark.parametrize("scale", [1e-20, 1e5])
def test_two_pieces_at_any_magnitude_of_the_diffs(aslp, dev, scale):
    """The loss's share of d_h scaled: [d_z | d_r] and d_m, the left operands of the backward products, are then 1e-20 or 1e5 times their usual
    size.  The backward buffer, divided by the scale, meets the bar of pieces 0 and 2 against the unscaled float64 reference."""
    k = next(i for i, c in enumerate(ref.CASES) if (c.H, c.S, c.T) == (132, 9, 3) and not c.windows)
    got = guarded((IDS[k], 2), lambda: ref.run_on_gpu(aslp, torch, dev, inputs(k), 2, 2, d_scale=scale))
    ry, rd = reference(k)
    assert np.isfinite(got["d"]).all()
    unscaled = dict(y=got["y"], d=got["d"].astype(np.float64) / scale)
    dist = ref.distances(ref.CASES[k], unscaled["y"], unscaled["d"], ry, rd)
    print("gru-seq %s [pieces 2, d_h x %g]: worst relative l2 %.2e, element %.2e" % (IDS[k], scale, max(v[0] for v in dist.values()), max(v[1] for v in dist.values())))
    ref.compare(inputs(k), unscaled, ry, rd, BAR0)


def test_probes_refuse_what_the_kernels_do_not_take(aslp, dev):
    """probes only: nothing is launched on refused arguments, under any piece count"""
    lib, GruSeq = aslp.lib, aslp._lib.GruSeq

    def probe(H, S, s_begin=0, s_count=0):
        q = GruSeq(None, None, None, None, 0, 0, 8 * H, 3, S, H, s_begin, s_count)   # (ld a multiple of 4 also at H = 6)
        return [lib.aslp_gru_seq_supported(C.byref(q), backward) for backward in (0, 1)]

    try:
        for pieces in ref.PIECES:
            lib.aslp_gru_seq_pieces(pieces)
            assert probe(512, 8) == [1, 1] and probe(4, 1) == [1, 1] and probe(512, 64) == [1, 1], pieces
            assert probe(516, 8) == [0, 0], pieces                       # more than 32 workgroups per chain
            assert probe(6, 8) == [0, 0], pieces                         # cells no multiple of 4
            assert probe(64, 65) == [0, 0], pieces                       # more than 8 chains
            assert probe(64, 20, 16, 5) == [0, 0] and probe(64, 20, 15, 5) == [1, 1], pieces   # s_begin + s_count > S
    finally:
        lib.aslp_gru_seq_pieces(-1)


CHILD = r'''
import sys
import numpy as np, torch
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import aslp_import
import gru_seq_ref as ref
aslp = aslp_import.load(); aslp.ops.use_torch_stream()
dev = torch.device("cuda:0")
k, want = int(sys.argv[2]), int(sys.argv[3])
assert aslp.lib.aslp_gru_seq_pieces_get() == want, aslp.lib.aslp_gru_seq_pieces_get()
got = ref.run_on_gpu(aslp, torch, dev, ref.build_case(ref.CASES[k]), -1, want)     # -1: the environment decides
np.savez(sys.argv[1], y=got["y"], d=got["d"])
'''


def run_child(request, tmp_path, env, k, want):
    """case k in a fresh interpreter under `env` (the parent, which has the GPU open, is not replaced)"""
    if first_failed_child or launch_failed:
        pytest.fail("not started: an earlier launch or child ended badly, and nothing more runs on the GPU behind it\n%s" % ((first_failed_child + launch_failed)[0],))
    out = str(tmp_path / ("child%d.npz" % want))
    e = dict(os.environ)
    e.pop("ASLP_GRU_SEQ_PIECES", None)
    e.update(env)
    try:
        p = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}, out, str(k), str(want)], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    except subprocess.TimeoutExpired as err:
        first_failed_child.append((request.node.name, "time limit of 300 s\n" + (err.stderr or b"").decode(errors="replace")[-2000:]))
        pytest.fail("child ran into its time limit")
    if p.returncode != 0:
        first_failed_child.append((request.node.name, "exit status %d\n%s" % (p.returncode, p.stderr.decode(errors="replace")[-3000:])))
        pytest.fail("child ended with status %d\n%s" % (p.returncode, p.stderr.decode(errors="replace")[-3000:]))
    res = np.load(out)
    return dict(y=res["y"], d=res["d"])


def test_switch_off_gives_the_bits_of_a_process_that_never_set_it(request, tmp_path, aslp, dev):
    """aslp_gru_seq_pieces(2) then (0): the bits of a fresh child with nothing set (which runs pieces 0); ASLP_GRU_SEQ_PIECES=1 in a fresh child
    selects one piece and gives the bits of aslp_gru_seq_pieces(1) here.  The children run one after the other."""
    k = next(i for i, c in enumerate(ref.CASES) if (c.H, c.S, c.T) == (132, 9, 3) and not c.windows)
    same = lambda a, b: np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
    assert os.environ.get("ASLP_GRU_SEQ_PIECES") is None and aslp.lib.aslp_gru_seq_pieces_get() == 0, "the suite runs with ASLP_GRU_SEQ_PIECES unset"
    gpu_run(aslp, dev, k, 2)
    aslp.lib.aslp_gru_seq_pieces(2); aslp.lib.aslp_gru_seq_pieces(0)
    off = guarded((IDS[k], 0), lambda: ref.run_on_gpu(aslp, torch, dev, inputs(k), 0, 0))
    fresh = run_child(request, tmp_path, {}, k, 0)
    assert same(off["y"], fresh["y"]) and same(off["d"], fresh["d"])
    assert same(off["y"], gpu_run(aslp, dev, k, 0)["y"]) and same(off["d"], gpu_run(aslp, dev, k, 0)["d"])
    one = run_child(request, tmp_path, {"ASLP_GRU_SEQ_PIECES": "1"}, k, 1)
    here = gpu_run(aslp, dev, k, 1)
    assert same(one["y"], here["y"]) and same(one["d"], here["d"])
    assert not same(one["y"], fresh["y"])


def test_bars_stay_four_times_above_what_was_measured():
    """The bar of pieces 0 and 2 against the errors this run saw (when the tests above ran in this process): at least 4 x above the pieces = 0
    kernels' worst, met by pieces = 2 as well, and never above the suite's fp32 bar of 1e-4."""
    assert BAR0[0] <= 1e-4 and BAR0[1] <= 1e-3
    for pieces in (0, 2):
        l2, el = MEASURED_WORST[pieces]
        assert l2 < BAR0[0] and el < BAR0[1], pieces
    assert 4 * MEASURED_WORST[0][0] <= BAR0[0] and 4 * MEASURED_WORST[0][1] <= BAR0[1]
    for pieces, (l2, el) in sorted(worst_seen.items()):
        print("gru-seq worst over all cases [pieces %d]: relative l2 %.2e, element %.2e" % (pieces, l2, el))
        if pieces == 0:
            assert 4 * l2 <= BAR0[0] and 4 * el <= BAR0[1], (pieces, l2, el)
