"""The CTC kernels of csrc/ctc.hip on the paths the rest of the suite does not reach, against the float64 model of tests/ctc_ref.py (pinned
to the reference's fixtures and measured against the oracle by tests/test_ctc_ref_cpu.py): every thread rung of ctc_lattice_kernel (64, 128,
256, 512) at its boundaries with a short utterance beside the long ones, every slot count 1..8 at both ends of the slot (L up to 2047), one
alignment exactly / none, an alphabet of 2, the tile softmax at one row per workgroup (A = 5088, 10175), the lane-per-row softmax (A = 10176,
and the rungs again in a child process under ASLP_CTC_SOFTMAX_TILED=0), utterances without a frame; the limits of the entry point; and the
two entry points the engine calls, aslp_ctc_loss_strided and aslp_eesen_ctc_mseq, on padded buffers whose padding is poisoned.

The bar comes from the oracle, never from the GPU: per utterance the GPU's distance to float64 (cost: relative; gradient rows t < T: relative
l2 and largest element difference) may be MARGIN x the distance of the oracle's fp32 restatement of the reference on that utterance, with
floors where fp32 is simply accurate (ctc_ref.FLOOR_*).  Beyond L ~ 128 an fp32 lattice cannot lie within 1e-4 of float64 (DESIGN section
7), so against the oracle directly the project's 1e-4 is asserted on the rungs group and wherever the oracle is within 1e-5 of float64, and
printed elsewhere.

Measured on an MI355X (MEASURED below): compute_ctc_loss and aslp_ctc_loss_strided lie where the oracle lies -- worst GPU / oracle ratio
1.00 in every group, their costs bit-identical to the oracle's and their gradients within 1.8e-6 relative l2 of the oracle's at every length
up to L = 2047 -- and aslp_eesen_ctc_mseq, which is handed fp32 probabilities and so rounds elsewhere, at 1.47 at the worst (slots-2-4,
L = 768).  Every ratio <= 1.5: MARGIN is 2.  The file takes 6.4 to 9.3 s, 1.9 s of it the child process."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import ctc_ref as ref
from test_oracle_ctc_cpu import orc_ctc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7.25            # what the padded gradient buffers hold before a call
STRIDED = ["rungs-256", "slots-2-4", "tight", "empty"]   # one rungs minibatch, the first slots minibatch, and the two with utterances no call may touch
_t0 = time.time()
_data, _gpu = {}, {}
launch_failed = []          # [(what, error)]: once a launch ended in an error, nothing further is started on the GPU
seen_shapes = {}            # case -> (threads, slot counts)
worst_ratio = {}            # case -> [cost, l2, element]: the GPU's distance to float64 over the oracle's

vp, ci = C.c_void_p, C.c_int
i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def data(oracle, name):
    """inputs, float64 result, oracle result and the oracle's distances of a case: computed once per module, shared, never modified"""
    if name not in _data:
        inp = ref.build(ref.BY_NAME[name])
        c64, g64 = ref.reference(inp.acts, inp.labels, inp.in_len)
        flat, lab_len = ref.flat_labels(inp)
        oc, og = orc_ctc(oracle, inp.acts.reshape(-1).copy(), flat, lab_len, inp.in_len, inp.A, inp.mb)
        og = og.reshape(inp.maxT, inp.mb, inp.A)
        _data[name] = (inp, c64, g64, oc, og, ref.distances(inp, oc, og, c64, g64))
    return _data[name]


def on_gpu(what, fn):
    """fn() behind the guard: an error other than a refused argument stops every later GPU call of this file"""
    if launch_failed:
        pytest.fail("not started: %s ended in an error, and nothing more runs on the GPU behind it\n%s" % launch_failed[0])
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    except RuntimeError as e:
        if "invalid value" not in str(e):
            launch_failed.append((what, repr(e)))
        raise
    except AssertionError:
        raise
    except Exception as e:
        launch_failed.append((what, repr(e)))
        raise


def loss(aslp, dev, inp, want_grad=True):
    costs, grads = aslp.ops.ctc_loss(torch.from_numpy(inp.acts).to(dev), inp.labels, inp.in_len, want_grad=want_grad)
    return costs, (grads.cpu().numpy().reshape(inp.maxT, inp.mb, inp.A) if want_grad else None)


def gpu(aslp, dev, oracle, name):
    if name not in _gpu:
        inp = data(oracle, name)[0]
        _gpu[name] = on_gpu(name, lambda: loss(aslp, dev, inp))
    return _gpu[name]


def untouched(inp, g, value):
    """rows t >= T, and every row of an utterance without an alignment, hold the bits they held before the call"""
    want = bits(np.float32(value))
    for n in range(inp.mb):
        T = int(inp.in_len[n]) if inp.feasible[n] else 0
        assert (bits(g[T:, n]) == want).all(), (inp.case.name, "utterance", n, "rows from", T)


def check_against_model(inp, what, costs, g, c64, g64, d_ref):
    """the float64-derived bar, per utterance; -> the distances"""
    d = ref.distances(inp, costs, g, c64, g64)
    worst = worst_ratio.setdefault(what, [0.0, 0.0, 0.0])
    for n in range(inp.mb):
        if not inp.feasible[n]:
            continue
        bar, r = ref.bars(d_ref[n]), ref.ratios(d[n], d_ref[n])
        for k in range(3):
            worst[k] = max(worst[k], r[k])
        print("ctc %-16s L %4d T %4d: cost %.2e (oracle %.2e)  l2 %.2e (%.2e)  element %.2e (%.2e)  ratios %.2f %.2f %.2f"
              % (what, len(inp.labels[n]), inp.in_len[n], d[n][0], d_ref[n][0], d[n][1], d_ref[n][1], d[n][2], d_ref[n][2], r[0], r[1], r[2]))
    for n in range(inp.mb):
        if inp.feasible[n]:
            bar = ref.bars(d_ref[n])
            assert d[n][0] <= bar[0] and d[n][1] <= bar[1] and d[n][2] <= bar[2], (what, "utterance", n, "L", len(inp.labels[n]), d[n], "bar", bar)
    return d


@pytest.mark.parametrize("name", ref.NAMES)
def test_case_matches_float64_model(aslp, oracle, dev, name):
    inp, c64, g64, oc, og, d_ref = data(oracle, name)
    threads, slots = ref.lattice_shape(inp)
    seen_shapes[name] = (threads, slots)
    print("\nctc %s: A %d, mb %d, maxT %d -> lat_threads %d, nslots %s" % (name, inp.A, inp.mb, inp.maxT, threads, slots))
    costs, g = gpu(aslp, dev, oracle, name)
    assert not np.isnan(costs).any() and not np.isnan(g).any()
    untouched(inp, g, 0.0)
    for n in range(inp.mb):
        if not inp.feasible[n]:
            assert bits(costs[n]) == 0, (name, n, costs[n])
    check_against_model(inp, name, costs, g, c64, g64, d_ref)
    # against the oracle directly, at the project's tolerance where fp32 can meet it
    for n in range(inp.mb):
        if inp.feasible[n]:
            T = int(inp.in_len[n])
            e = oracle.rel_err(g[:T, n], og[:T, n])
            ec = abs(float(costs[n]) - float(oc[n])) / max(abs(float(oc[n])), 1e-30)
            asserted = inp.case.group == "rungs" or d_ref[n][1] <= 1e-5
            print("ctc %-16s L %4d against the oracle: cost %.2e, gradient %.2e%s" % (name, len(inp.labels[n]), ec, e, "" if asserted else "  (not asserted)"))
            if asserted:
                assert e < 1e-4 and ec < 1e-4, (name, n, e, ec)
    if name == "tight":   # exactly one alignment: the cost has a closed form that no lattice enters
        closed = ref.closed_form_cost(inp.acts, 0, inp.mb, inp.paths[0])
        assert abs(float(costs[0]) - closed) / closed <= ref.bars(d_ref[0])[0], (float(costs[0]), closed)


def test_scores_only_gives_the_same_costs(aslp, oracle, dev):
    for name in [n for n in ref.NAMES if ref.BY_NAME[n].group == "rungs"] + ["slots-2-4"]:
        inp = data(oracle, name)[0]
        costs, grads = on_gpu(name + " scores only", lambda: loss(aslp, dev, inp, want_grad=False))
        assert grads is None and np.array_equal(bits(costs), bits(gpu(aslp, dev, oracle, name)[0])), name


def test_second_call_gives_the_same_bits(aslp, oracle, dev):
    name = "slots-6-8"
    inp = data(oracle, name)[0]
    first = gpu(aslp, dev, oracle, name)
    costs, g = on_gpu(name + " again", lambda: loss(aslp, dev, inp))
    assert np.array_equal(bits(costs), bits(first[0])) and np.array_equal(bits(g), bits(first[1]))


def test_limits_of_the_entry_point(aslp, oracle, dev):
    assert 8 in ref.lattice_shape(data(oracle, "slots-6-8")[0])[1] and max(len(l) for l in data(oracle, "slots-6-8")[0].labels) == 2047
    gpu(aslp, dev, oracle, "slots-6-8")                         # L = 2047 ran
    rng = np.random.default_rng(61)
    lab = [1 + (i % 2) for i in range(2048)]                    # no repeats: T = L = 2048 has an alignment, 8 slots of 512 threads do not hold it
    acts = torch.from_numpy(rng.standard_normal((2048, 3)).astype(np.float32)).to(dev)
    with pytest.raises(RuntimeError, match="invalid value"):
        on_gpu("L = 2048", lambda: aslp.ops.ctc_loss(acts, [lab], [2048]))
    big = ref.custom("alphabet-10240", 10240, [ref.Utt(1, 0, 5)], 62)    # the gradient kernel's LDS: 4 x (S + A) floats and the label tables
    with pytest.raises(RuntimeError, match="invalid value"):
        on_gpu("A = 10240", lambda: loss(aslp, dev, big))
    # scores only there is no gradient kernel and no limit on the alphabet
    wide = ref.custom("alphabet-12000", 12000, [ref.Utt(0, 0, 5), ref.Utt(1, 0, 5), ref.Utt(2, 0, 5)], 63)
    costs, _ = on_gpu("A = 12000 scores only", lambda: loss(aslp, dev, wide, want_grad=False))
    c64, _ = ref.reference(wide.acts, wide.labels, wide.in_len)
    flat, lab_len = ref.flat_labels(wide)
    oc, _ = orc_ctc(oracle, wide.acts.reshape(-1).copy(), flat, lab_len, wide.in_len, wide.A, wide.mb, want_grad=False)
    for n in range(wide.mb):
        d_ref = abs(float(oc[n]) - c64[n]) / abs(c64[n])
        assert abs(float(costs[n]) - c64[n]) / abs(c64[n]) <= max(ref.MARGIN * d_ref, ref.FLOOR_COST), (n, costs[n], c64[n], d_ref)


def padded_call(aslp, dev, fn_name, inp, x, ld_x, ld_g):
    """aslp_ctc_loss_strided / aslp_eesen_ctc_mseq on row-padded device buffers: the input's padding NaN, the output prefilled with SENTINEL;
    -> (per-utterance result, output buffer [maxT, mb, ld_g])"""
    fn = getattr(aslp.lib, fn_name)
    fn.restype = ci
    fn.argtypes = [vp, ci, vp, ci, i32p, i32p, i32p, ci, ci, f32p]
    rows = inp.maxT * inp.mb
    xp = np.full((rows, ld_x), np.nan, np.float32)
    xp[:, :inp.A] = x
    xd = torch.from_numpy(xp).to(dev)
    gd = torch.full((rows, ld_g), SENTINEL, dtype=torch.float32, device=dev)
    flat, lab_len = ref.flat_labels(inp)
    per_utt = np.full(inp.mb, np.nan, np.float32)

    def run():
        st = fn(xd.data_ptr(), ld_x, gd.data_ptr(), ld_g, flat, lab_len, np.ascontiguousarray(inp.in_len, np.int32), inp.A, inp.mb, per_utt)
        if st != 0:
            raise RuntimeError("%s: %s" % (fn_name, aslp.lib.ctcGetStatusString(st).decode()))
        aslp.check_error()
    on_gpu("%s on %s" % (fn_name, inp.case.name), run)
    return per_utt, gd.cpu().numpy().reshape(inp.maxT, inp.mb, ld_g)


@pytest.mark.parametrize("name", STRIDED)
def test_strided_entry_point_on_poisoned_padding(aslp, oracle, dev, name):
    inp = data(oracle, name)[0]
    costs, g = gpu(aslp, dev, oracle, name)
    A = inp.A
    scosts, sg = padded_call(aslp, dev, "aslp_ctc_loss_strided", inp, inp.acts, A + 3, A + 9)
    assert np.array_equal(bits(scosts), bits(costs))
    assert (bits(sg[:, :, A:]) == bits(np.float32(SENTINEL))).all()          # padding columns
    untouched(inp, sg[:, :, :A], SENTINEL)
    for n in range(inp.mb):
        T = int(inp.in_len[n]) if inp.feasible[n] else 0
        assert np.array_equal(bits(sg[:T, n, :A]), bits(g[:T, n])), (name, n)


@pytest.mark.parametrize("name", STRIDED)
def test_eesen_entry_point_on_poisoned_padding(aslp, oracle, dev, name):
    """post-softmax outputs in, diff = y - posterior and log p(z|x) out: the Warp-CTC gradient and -cost of the same utterances"""
    inp, _, _, _, _, d_ref = data(oracle, name)
    A = inp.A
    probs = np.exp(ref.log_softmax(inp.acts)).astype(np.float32)
    c64, g64 = ref.reference(probs, inp.labels, inp.in_len, probs=True)      # float64 on the fp32 outputs the entry point is given
    pzx, diff = padded_call(aslp, dev, "aslp_eesen_ctc_mseq", inp, probs, A + 3, A + 9)
    assert (bits(diff[:, :, A:]) == bits(np.float32(SENTINEL))).all()
    untouched(inp, diff[:, :, :A], SENTINEL)
    for n in range(inp.mb):
        if not inp.feasible[n]:
            assert bits(pzx[n]) == bits(np.float32(-1e30)), (name, n, pzx[n])
    assert not np.isnan(pzx).any() and not np.isnan(diff[:, :, :A]).any()
    costs = np.where(inp.feasible, -pzx, 0.0).astype(np.float32)
    check_against_model(inp, name + " eesen", costs, diff[:, :, :A], c64, g64, d_ref)


CHILD = r'''
import sys
import numpy as np, torch
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import aslp_import
import ctc_ref as ref
aslp = aslp_import.load(); aslp.ops.use_torch_stream()
dev = torch.device("cuda:0")
out = []
for name in sys.argv[2:]:
    inp = ref.build(ref.BY_NAME[name])
    costs, grads = aslp.ops.ctc_loss(torch.from_numpy(inp.acts).to(dev), inp.labels, inp.in_len)
    torch.cuda.synchronize()
    out += [np.asarray(costs, np.float32).ravel(), grads.cpu().numpy().ravel()]
np.save(sys.argv[1], np.concatenate(out))
'''


def test_lane_per_row_softmax_gives_the_tile_kernels_bits(aslp, oracle, dev, tmp_path):
    """ASLP_CTC_SOFTMAX_TILED=0 is read once per process: the rungs group in one fresh child process (it stops at its first error).  Both
    softmax kernels claim the reference's exact arithmetic, so every cost and gradient has the bits of this process' run."""
    assert os.environ.get("ASLP_CTC_SOFTMAX_TILED", "1")[0] != "0", "this process must run the tile kernel"
    names = [n for n in ref.NAMES if ref.BY_NAME[n].group == "rungs"]
    here = np.concatenate([a.ravel() for n in names for a in gpu(aslp, dev, oracle, n)])
    if launch_failed:
        pytest.fail("not started: %s ended in an error, and nothing more runs on the GPU behind it\n%s" % launch_failed[0])
    out = str(tmp_path / "lane_per_row.npy")
    env = dict(os.environ, ASLP_CTC_SOFTMAX_TILED="0")
    try:
        p = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}, out] + names, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    except subprocess.TimeoutExpired as err:
        launch_failed.append(("the lane-per-row child", "time limit of 120 s\n" + (err.stderr or b"").decode(errors="replace")[-2000:]))
        pytest.fail("child ran into its time limit")
    if p.returncode != 0:
        launch_failed.append(("the lane-per-row child", "exit status %d\n%s" % (p.returncode, p.stderr.decode(errors="replace")[-3000:])))
        pytest.fail("child ended with status %d\n%s" % (p.returncode, p.stderr.decode(errors="replace")[-3000:]))
    there = np.load(out)
    assert there.shape == here.shape and np.array_equal(bits(there), bits(here))


# GPU distance / oracle distance to float64 (cost, gradient l2, gradient element), worst utterance per case, on an MI355X; the file's time
MEASURED = {
    "rungs-64": (0.34, 0.40, 0.41), "rungs-128": (0.42, 1.00, 1.00), "rungs-256": (0.43, 1.00, 1.00), "rungs-512": (0.22, 1.00, 1.00),
    "slots-2-4": (1.00, 1.00, 1.00), "slots-4-6": (1.00, 1.00, 1.00), "slots-6-8": (1.00, 1.00, 1.00), "tight": (0.59, 1.00, 1.00),
    "alphabet-2": (0.21, 0.57, 0.23), "alphabet-5088": (0.04, 0.60, 1.00), "alphabet-10175": (0.37, 0.69, 1.00),
    "alphabet-10176": (0.41, 0.25, 0.64), "empty": (0.01, 0.03, 0.02),
    "rungs-256 eesen": (0.43, 1.38, 1.00), "slots-2-4 eesen": (1.32, 1.47, 1.25), "tight eesen": (0.43, 1.24, 1.25), "empty eesen": (0.08, 0.02, 0.02),
}
MEASURED_SECONDS = (6.4, 9.3)   # two runs


def test_report_rungs_slots_and_ratios():
    """what ran (when the tests above ran in this process), and how the GPU's distance to float64 compares with the oracle's"""
    print()
    for name, (threads, slots) in seen_shapes.items():
        print("ctc %-16s lat_threads %3d nslots %s" % (name, threads, slots))
    for name, r in worst_ratio.items():
        print("ctc %-22s GPU / oracle distance to float64: cost %.2f, l2 %.2f, element %.2f" % ((name,) + tuple(r)))
    if worst_ratio:
        print("ctc worst ratio over all cases: %.2f (margin %.1f)" % (max(max(r) for r in worst_ratio.values()), ref.MARGIN))
    print("ctc edges: %.1f s since the module was imported" % (time.time() - _t0))
    if len(seen_shapes) == len(ref.NAMES):
        assert {t for t, _ in seen_shapes.values()} == {64, 128, 256, 512}
        assert set().union(*[s for t, s in seen_shapes.values() if t == 512]) == set(range(1, ref.LAT_SLOTS + 1))
    for name, r in MEASURED.items():
        assert max(r) <= ref.MARGIN, (name, r)
