"""The 36 persistent LSTM kernels of csrc/rnn_persistent.hip (lstm_seq_fwd, lstm_seq_fwd_h, lstm_seq_bwd, lstm_seq_bwd_h over coupled gates,
the cell-count rungs, exact / fast activations and one / two fp16 pieces) against the float64 model of the aslp_lstm_seq contract
(tests/lstm_seq_ref.py, pinned to the oracle by tests/test_lstm_seq_ref_cpu.py, which also counts that the cases below launch all 36).

aslp_lstm_seq_forward / _backward are driven through the C ABI on padded buffers (ld = (G+3) C + 8, ldw = C + 4, grad_ld = C + 4), every
case under the default switches, aslp_lstm_split16(0) and aslp_lstm_operand_pieces(1); after every launch the error state, which kernel
family ran, and bit for bit everything the launch must not write (lstm_seq_ref.run_on_gpu).  Then tensor by tensor and per direction --
gate, c, h, m columns; d gate columns, d_c, d_h; every grad_partial row of every active chain -- against float64:
  two fp16 pieces, the fp32 instruction, exact activations:  relative l2 error < 1e-5 per tensor, element error < 1e-4 of max(1, largest |reference|)
  one fp16 piece:                                            2e-3 / 2e-2, and not the bits of the two-piece run
The environment switches are read once per process: ASLP_LSTM_FAST_ACT=0 (the twelve exact-activation kernels) and ASLP_LSTM_WAVE_COLLECT=0
ASLP_LSTM_READ_AHEAD=0 (bit-identical to the default) each run the whole list in one child process, one after the other.

Measured on an MI355X, worst over all cases (relative l2 / element): two pieces 4.5e-7 / 4.4e-7, the fp32 instruction 4.5e-7 / 5.3e-7, exact
activations 4.0e-7 / 8.1e-7 -- the bar of 1e-5 / 1e-4 stands 12 x above the worst of them, so it is kept as it is; one piece 2.5e-4 / 1.1e-3
against 2e-3 / 2e-2 (MEASURED_WORST below).  The file takes 7.5 s, 4.7 s of it the two child processes."""
import os
import subprocess
import sys

import ctypes as C
import numpy as np
import pytest
import torch

import lstm_seq_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [ref.case_id(c) for c in ref.CASES]
_inputs, _refs, _runs = {}, {}, {}
worst_seen = {}          # switch label -> [l2, element], for the report at the end of the file's run
launch_failed = []       # [(case, switch, error)]: once a launch ended in an error, nothing further is launched
first_failed_child = []  # once a child ended badly, no further child is started


def inputs(k):
    if k not in _inputs:
        _inputs[k] = ref.build_case(ref.CASES[k])
    return _inputs[k]


def reference(k):
    """the float64 run of case k: computed once, shared, never modified"""
    if k not in _refs:
        _refs[k] = ref.reference(inputs(k))
    return _refs[k]


def gpu_run(aslp, dev, k, switch):
    if (k, switch) not in _runs:
        if launch_failed:
            pytest.fail("not started: a launch of %s [%s] ended in an error, and nothing more runs on the GPU behind it\n%s" % launch_failed[0])
        label, split16, pieces, want = next(s for s in ref.SWITCHES if s[0] == switch)
        try:
            _runs[(k, switch)] = ref.run_on_gpu(aslp, torch, dev, inputs(k), split16, pieces, want)
        except AssertionError:
            raise
        except Exception as e:   # the library's error state (a spin limit, a failed launch) or the runtime's
            launch_failed.append((IDS[k], switch, repr(e)))
            raise
    return _runs[(k, switch)]


def note(label, worst):
    w = worst_seen.setdefault(label, [0.0, 0.0])
    w[0], w[1] = max(w[0], worst[0]), max(w[1], worst[1])


def check_dmax(k, got):
    """the per-workgroup maxima a single launch of the fp16 kernels leaves: their maximum per direction is the largest finite |dGATES| of that
    direction as the GPU wrote it, exactly"""
    c = ref.CASES[k]
    for launch, nd in enumerate(got["last_dmax"]):
        if nd > 0:
            for d in range(c.ndir):
                assert float(got["dmax"][launch][d].max()) == ref.dmax(inputs(k), got["d"][d]), (IDS[k], "direction", d)


@pytest.mark.parametrize("switch", [s[0] for s in ref.SWITCHES])
@pytest.mark.parametrize("k", range(len(ref.CASES)), ids=IDS)
def test_kernels_match_float64_model(aslp, dev, k, switch):
    got = gpu_run(aslp, dev, k, switch)
    ys, ds, parts = reference(k)
    worst = ref.compare(inputs(k), got, ys, ds, parts, ref.BAR_ONE_PIECE if switch == "pieces=1" else ref.BAR)
    note(switch, worst)
    print("lstm-seq %s [%s]: worst relative l2 %.2e, element %.2e" % (IDS[k], switch, worst[0], worst[1]))
    check_dmax(k, got)
    c = ref.CASES[k]
    if switch == "pieces=1" and not (c.T == 1 and (c.skip or c.k_first)):   # (without a recurrent product there is nothing the pieces change)
        two = gpu_run(aslp, dev, k, "default")
        assert not all(np.array_equal(a, b) for a, b in zip(got["y"] + got["d"], two["y"] + two["d"])), (IDS[k], "one piece gave the two-piece bits")


def test_probes_refuse_what_the_kernels_do_not_take(aslp, dev):
    """probes only: nothing is launched on refused arguments"""
    lib, Seq = aslp.lib, aslp._lib.Seq

    def probe(Cc, S, ndir=1, s_begin=0, s_count=0):
        a = Seq()
        a.ndir, a.ld, a.ldw, a.T, a.S, a.C, a.cifg, a.s_begin, a.s_count = ndir, 8 * Cc, 2 * Cc, 3, S, Cc, 0, s_begin, s_count   # (ld, ldw multiples of 4 also at C = 6)
        return [lib.aslp_lstm_seq_supported(C.byref(a), backward) for backward in (0, 1)]

    assert probe(512, 8) == [1, 1] and probe(4, 1) == [1, 1]
    assert probe(516, 8) == [0, 0]                       # more than 32 workgroups per chain
    assert probe(6, 8) == [0, 0]                         # cells no multiple of 4
    assert probe(64, 20, s_begin=16, s_count=5) == [0, 0] and probe(64, 20, s_begin=15, s_count=5) == [1, 1]   # s_begin + s_count > S
    assert probe(64, 33, ndir=2) == [0, 0] and probe(64, 32, ndir=2) == [1, 1] and probe(64, 65) == [0, 0]
    for k_first, Cc, ok in ((4, 4, 1), (128, 128, 1), (132, 128, 0), (256, 132, 1), (260, 512, 0), (6, 64, 0), (0, 64, 0)):
        assert lib.aslp_lstm_seq_first_product_supported_for(k_first, Cc) == ok, (k_first, Cc)


CHILD = r'''
import sys
import numpy as np, torch
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import aslp_import
import lstm_seq_ref as ref
aslp = aslp_import.load(); aslp.ops.use_torch_stream()
dev = torch.device("cuda:0")
res = {}
for k, case in enumerate(ref.CASES):
    inp = ref.build_case(case)
    for label, split16, pieces, want in ref.SWITCHES:
        if label in sys.argv[2:]:
            got = ref.run_on_gpu(aslp, torch, dev, inp, split16, pieces, want)
            for d in range(case.ndir):
                res["%%d|%%s|y%%d" %% (k, label, d)] = got["y"][d]
                res["%%d|%%s|d%%d" %% (k, label, d)] = got["d"][d]
            for n, part in enumerate(got["parts"]):
                res["%%d|%%s|p%%d" %% (k, label, n)] = part
            res["%%d|%%s|last_dmax" %% (k, label)] = np.asarray(got["last_dmax"], np.int32)
            for n, pair in enumerate(got["dmax"]):
                for d in range(2):
                    res["%%d|%%s|m%%d_%%d" %% (k, label, n, d)] = pair[d]
np.savez(sys.argv[1], **res)
'''


def run_child(request, tmp_path, env, switches):
    """the whole case list in a fresh interpreter under `env` (the parent, which has the GPU open, is not replaced); -> per (case, switch) what
    run_on_gpu returned there"""
    if first_failed_child:
        pytest.fail("not started: the child of %s ended badly, and nothing more runs on the GPU behind it\n%s" % first_failed_child[0])
    out = str(tmp_path / "child.npz")
    e = dict(os.environ)
    for name in ("ASLP_LSTM_FAST_ACT", "ASLP_LSTM_WAVE_COLLECT", "ASLP_LSTM_READ_AHEAD", "ASLP_LSTM_SPLIT_F16", "ASLP_LSTM_PIECES"):
        e.pop(name, None)
    e.update(env)
    try:
        p = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}, out] + list(switches), env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    except subprocess.TimeoutExpired as err:
        first_failed_child.append((request.node.name, "time limit of 300 s\n" + (err.stderr or b"").decode(errors="replace")[-2000:]))
        pytest.fail("child ran into its time limit")
    if p.returncode != 0:
        first_failed_child.append((request.node.name, "exit status %d\n%s" % (p.returncode, p.stderr.decode(errors="replace")[-3000:])))
        pytest.fail("child ended with status %d\n%s" % (p.returncode, p.stderr.decode(errors="replace")[-3000:]))
    res = np.load(out)
    runs = {}
    for k, c in enumerate(ref.CASES):
        for label in switches:
            nl = len(ref.launches(c))
            runs[(k, label)] = dict(y=[res["%d|%s|y%d" % (k, label, d)] for d in range(c.ndir)], d=[res["%d|%s|d%d" % (k, label, d)] for d in range(c.ndir)],
                                    parts=[res["%d|%s|p%d" % (k, label, n)] for n in range(nl)], last_dmax=[int(v) for v in res["%d|%s|last_dmax" % (k, label)]],
                                    dmax=[[res["%d|%s|m%d_%d" % (k, label, n, d)] for d in range(2)] for n in range(nl)])
    return runs


def test_exact_activation_kernels_match_float64_model(request, tmp_path):
    """ASLP_LSTM_FAST_ACT=0: lstm_seq_fwd<., ., false> and lstm_seq_fwd_h<., ., false, .> (twelve kernels), every case under every switch"""
    switches = [s[0] for s in ref.SWITCHES]
    runs = run_child(request, tmp_path, {"ASLP_LSTM_FAST_ACT": "0"}, switches)
    for (k, label), got in sorted(runs.items()):
        ys, ds, parts = reference(k)
        worst = ref.compare(inputs(k), got, ys, ds, parts, ref.BAR_ONE_PIECE if label == "pieces=1" else ref.BAR)
        note("exact activations, " + label, worst)
        check_dmax(k, got)
    for label in switches:
        print("lstm-seq ASLP_LSTM_FAST_ACT=0 [%s]: worst relative l2 %.2e, element %.2e" % ((label,) + tuple(worst_seen["exact activations, " + label])))


def test_collection_switches_change_no_bit(request, tmp_path, aslp, dev):
    """ASLP_LSTM_WAVE_COLLECT=0 ASLP_LSTM_READ_AHEAD=0 change when operands are fetched, not what is multiplied: every buffer of every case,
    two-piece and fp32-instruction kernels alike, has the bits of this process' default run"""
    switches = ["default", "split16=0"]
    runs = run_child(request, tmp_path, {"ASLP_LSTM_WAVE_COLLECT": "0", "ASLP_LSTM_READ_AHEAD": "0"}, switches)
    for (k, label), got in sorted(runs.items()):
        here = gpu_run(aslp, dev, k, label)
        same = lambda a, b: np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
        for name in ("y", "d", "parts"):
            assert len(got[name]) == len(here[name]) and all(same(a, b) for a, b in zip(got[name], here[name])), (IDS[k], label, name)
        assert got["last_dmax"] == here["last_dmax"]
        assert all(same(a, b) for p, q in zip(got["dmax"], here["dmax"]) for a, b in zip(p, q)), (IDS[k], label, "dmax_parts")


# worst relative l2 / element error over all cases on an MI355X, per switch (printed again by the test below)
MEASURED_WORST = {"default": (4.45e-07, 4.36e-07), "split16=0": (4.45e-07, 5.30e-07), "pieces=1": (2.48e-04, 1.10e-03),
                  "exact activations, default": (4.00e-07, 8.14e-07), "exact activations, split16=0": (4.00e-07, 7.00e-07),
                  "exact activations, pieces=1": (2.49e-04, 1.10e-03)}


def test_bars_stay_four_times_above_what_was_measured():
    """The bars against the errors this run saw (when the tests above ran in this process): at least 4 x above, so that another box does not
    flip them, and never above the suite's fp32 bar of 1e-4."""
    assert ref.BAR <= 1e-4 and ref.BAR_ONE_PIECE == 2e-3
    for label, (l2, el) in MEASURED_WORST.items():
        bar = ref.BAR_ONE_PIECE if "pieces=1" in label else ref.BAR
        assert l2 < bar and el < 10 * bar and ("pieces=1" in label or (4 * l2 <= bar and 4 * el <= 10 * bar)), label
    for label, (l2, el) in sorted(worst_seen.items()):
        print("lstm-seq worst over all cases [%s]: relative l2 %.2e, element %.2e" % (label, l2, el))
        bar = ref.BAR_ONE_PIECE if "pieces=1" in label else ref.BAR
        if "pieces=1" not in label:
            assert 4 * l2 <= bar and 4 * el <= 10 * bar, (label, l2, el)
