"""Mse through the engine: the Python class and the C ABI under it (aslp_mse_*), Nnet.train_step_mse, the A/B switch ASLP_MSE_FUSED and
MultiTaskLoss' mse task, against tests/mse_ref.py and against the reference's op sequence the switch gives back."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import kaldi_formats as kf
import mse_engine_steps as steps
import mse_ref
import nnet_io

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kaldi-aslp_amd", "bin")


@pytest.fixture(scope="module")
def fused(aslp, dev):
    """the steps of tests/mse_engine_steps.py in this process: the default, one launch per Eval"""
    assert os.environ.get("ASLP_MSE_FUSED", "1") != "0", "this module compares the default with ASLP_MSE_FUSED=0: run it without the switch"
    return steps.run_all(aslp, dev)


@pytest.fixture(scope="module")
def op_sequence(tmp_path_factory):
    """... and in a fresh child process under ASLP_MSE_FUSED=0 (the switch is read once per process)"""
    out = str(tmp_path_factory.mktemp("mse_ab") / "ops.npz")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mse_engine_steps.py"), out], env=dict(os.environ, ASLP_MSE_FUSED="0"),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return dict(np.load(out))


def test_mse_class_three_minibatches(aslp, dev):
    rows, cols = 4, 6
    w = np.array([0.5, 1.0, 1.0, 0.0], np.float32)   # 2.5 per batch: frames are truncated per minibatch, 3 x 2 = 6 and not int(7.5)
    mse = aslp.Mse()
    loss = 0.0
    for b in range(3):
        y, t, _ = mse_ref.inputs(rows, cols, 40 + b)
        want, _, total = mse_ref.model(y, t, w)
        loss += 0.5 * total
        diff = torch.empty((rows, cols), dtype=torch.float32, device=dev)
        mse.Eval(torch.from_numpy(w).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(t).to(dev), diff)
        assert np.array_equal(diff.cpu().numpy().view(np.uint32), want.view(np.uint32))
    st = mse.GetStats()
    assert st["frames"] == 6.0 and st["num_tgt"] == cols
    assert abs(st["loss"] - loss) <= mse_ref.total_bound(rows, cols) * loss
    rms = np.float32(np.sqrt(loss / 6.0 / cols))
    assert mse.Report() == "AvgLoss: %g (Mse), [RMS %g, frames 6]\n" % (loss / 6.0, rms)
    # frame_weights=None: ones
    y, t, _ = mse_ref.inputs(rows, cols, 50)
    want, _, total = mse_ref.model(y, t, np.ones(rows, np.float32))
    diff = torch.empty((rows, cols), dtype=torch.float32, device=dev)
    mse.Eval(None, torch.from_numpy(y).to(dev), torch.from_numpy(t).to(dev), diff)
    assert np.array_equal(diff.cpu().numpy().view(np.uint32), want.view(np.uint32))
    st2 = mse.GetStats()
    assert st2["frames"] == 10.0 and abs(st2["loss"] - (loss + 0.5 * total)) <= mse_ref.total_bound(rows, cols) * (loss + 0.5 * total)


def test_no_host_read_until_stats(aslp, dev):
    """ten Eval calls and ten whole training steps read nothing back; the first GetStats does.  (On the reference's op sequence every Eval
    reads its sum: this is the test that fails there.)"""
    cfg = steps.SMALL
    net = aslp.Nnet.Init(steps.proto(cfg["dims"], cfg["act"]), seed=1)
    net.SetTrainOptions(learn_rate=0.01, momentum=0.0)
    mse = aslp.Mse()
    x, t, w = steps.batches(cfg)[0]
    xd, td, wd = torch.from_numpy(x).to(dev), torch.from_numpy(t).to(dev), torch.from_numpy(w).to(dev)
    y = net.Propagate(xd)
    diff = torch.empty_like(y)
    mse.Eval(wd, y, td, diff)          # (first use: buffers are made)
    net.train_step_mse(mse, xd, td, wd)
    before = aslp.ops.device_to_host_syncs()
    for _ in range(10):
        mse.Eval(wd, y, td, diff)
    for _ in range(10):
        net.train_step_mse(mse, xd, td, wd)
    assert aslp.ops.device_to_host_syncs() == before
    st = mse.GetStats()
    assert aslp.ops.device_to_host_syncs() > before
    assert st["frames"] == 22 * mse_ref.num_frames(w) and np.isfinite(st["loss"])


def test_train_step_matches_composed_and_op_sequence(fused, op_sequence):
    """12 -> 16 Sigmoid -> 10 linear, two steps: train_step_mse, the step composed by hand from aslp_nnet_propagate + aslp_mse_eval_batch +
    aslp_nnet_backpropagate, and both again on the reference's op sequence leave the same parameters bit for bit"""
    base = fused["small_step_params"]
    assert np.isfinite(base).all() and not np.array_equal(base[0], base[1])
    for name, got in (("composed", fused["small_composed_params"]), ("ops step", op_sequence["small_step_params"]),
                      ("ops composed", op_sequence["small_composed_params"])):
        assert np.array_equal(base.view(np.uint32), got.view(np.uint32)), name
    rows, cols = steps.SMALL["rows"], steps.SMALL["dims"][2]
    a, b = fused["small_step_stats"], op_sequence["small_step_stats"]
    assert a[0] == b[0] and a[2] == b[2] == cols
    assert a[0] == sum(mse_ref.num_frames(w) for _, _, w in steps.batches(steps.SMALL))
    print("loss one launch %.17g, op sequence %.17g" % (a[1], b[1]))
    assert abs(a[1] - b[1]) <= 2 * mse_ref.total_bound(rows, cols) * b[1]
    assert np.array_equal(fused["small_composed_stats"], a)


def test_split16_output_layer_both_modes(fused, op_sequence):
    """rows 128, 128 -> 256 -> 128: the output layer's backward products run on the split-fp16 kernels, whose out-diff planes are scaled by
    the diff's maximum -- from the loss kernel's per-workgroup maxima (one launch), or from the conversion's own maximum pass (op sequence).
    Both are the exact maximum of the same diff, so nothing needs to differ; the bar is that of tests/test_dnn_ab_switches_gpu.py for a
    power-of-two scale that moves, 2e-6 per tensor, relative.  When run on an MI355X, both of the two steps came out bit-identical."""
    a, b = fused["split16_step_params"], op_sequence["split16_step_params"]
    assert np.isfinite(a).all()
    d_in, hid, out = steps.SPLIT16["dims"]
    print("steps bit-identical between the modes: %d of %d" % (sum(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b)), len(a)))
    for s in range(len(a)):
        o = 0
        for n in (hid * d_in, hid, out * hid, out):
            ta, tb = a[s, o:o + n].astype(np.float64), b[s, o:o + n].astype(np.float64)
            assert np.linalg.norm(ta - tb) <= 2e-6 * np.linalg.norm(tb), (s, o)
            o += n
        assert o == a.shape[1]
    la, lb = fused["split16_step_stats"], op_sequence["split16_step_stats"]
    assert la[0] == lb[0] and abs(la[1] - lb[1]) <= 2e-6 * lb[1]


def test_multitask_unaligned_window_both_modes(aslp, dev, tmp_path):
    """aslp-nnet-train-simple with multitask,xent,7,1.0,mse,5,0.25: the mse task's window starts at column 7 of the 12-column diff (the
    one-column access path, the task weight as the kernel's second rounding); the written model is byte-identical to the op sequence's"""
    rng = np.random.default_rng(77)
    D, H, D1, D2, mb = 12, 24, 7, 5, 16
    W1, b1 = rng.standard_normal((H, D)).astype(np.float32) * 0.3, rng.standard_normal(H).astype(np.float32) * 0.1
    W2, b2 = rng.standard_normal((D1 + D2, H)).astype(np.float32) * 0.3, rng.standard_normal(D1 + D2).astype(np.float32) * 0.1
    nnet_io.write_simple_nnet(tmp_path / "m.nnet", [("<AffineTransform>", D, H, nnet_io.affine(W1, b1)), ("<Sigmoid>", H, H, b""),
                                                     ("<AffineTransform>", H, D1 + D2, nnet_io.affine(W2, b2)),
                                                     ("<Sigmoid>", D1 + D2, D1 + D2, b"")])
    keys = ["mt%02d" % i for i in range(5)]
    lens = [int(x) for x in rng.integers(12, 40, len(keys))]
    feats = [rng.standard_normal((n, D)).astype(np.float32) for n in lens]
    posts = [[[(int(rng.integers(0, D1)), 1.0)] + [(D1 + c, float(np.float32(rng.uniform(0.05, 0.95)))) for c in range(D2)] for _ in range(n)]
             for n in lens]
    fws = [rng.choice(np.array([0.0, 1.0, 1.0, 2.0], np.float32), n) for n in lens]
    (tmp_path / "f.ark").write_bytes(kf.archive([(k, kf.matrix_bin(f)) for k, f in zip(keys, feats)]))
    (tmp_path / "p.ark").write_bytes(kf.archive([(k, kf.posterior_bin(p)) for k, p in zip(keys, posts)]))
    (tmp_path / "w.ark").write_bytes(kf.archive([(k, kf.vector_bin(x)) for k, x in zip(keys, fws)]))
    exe = os.path.join(BIN, "aslp-nnet-train-simple")
    assert os.path.exists(exe), "%s not built (make -C kaldi-aslp_amd)" % exe
    logs = {}
    for mode in ("1", "0"):
        p = subprocess.run([exe, "--objective-function=multitask,xent,%d,1.0,mse,%d,0.25" % (D1, D2), "--learn-rate=0.02", "--momentum=0.5",
                            "--minibatch-size=%d" % mb, "--randomize=false", "--frame-weights=ark:%s" % (tmp_path / "w.ark"),
                            "ark:%s" % (tmp_path / "f.ark"), "ark:%s" % (tmp_path / "p.ark"), str(tmp_path / "m.nnet"), str(tmp_path / ("out%s.nnet" % mode))],
                           env=dict(os.environ, ASLP_MSE_FUSED=mode), capture_output=True, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-3000:]
        logs[mode] = p.stderr.decode()
    one, ops = (tmp_path / "out1.nnet").read_bytes(), (tmp_path / "out0.nnet").read_bytes()
    assert one == ops and one != (tmp_path / "m.nnet").read_bytes()
    rx = r"Loss 2, AvgLoss: (\S+) \(Mse\), \[RMS (\S+), frames (\S+)\]"
    m1, m0 = re.search(rx, logs["1"]), re.search(rx, logs["0"])
    assert m1 and m0 and m1.group(3) == m0.group(3)
    assert abs(float(m1.group(1)) - float(m0.group(1))) <= 2e-5 * float(m0.group(1))   # (six printed digits)


def test_nan_target_is_a_host_error_at_the_fetch(aslp, dev):
    rows, cols = 8, 5
    y, t, w = mse_ref.inputs(rows, cols, 9)
    w[:] = 1.0
    t[3, 2] = np.nan
    h = aslp.nnet._H()
    assert aslp.lib.aslp_mse_create(aslp.nnet.C.byref(h)) == 0
    try:
        yd, td, wd = torch.from_numpy(y).to(dev), torch.from_numpy(t).to(dev), torch.from_numpy(w).to(dev)
        diff = torch.empty_like(yd)
        p = aslp.ops.ptr
        assert aslp.lib.aslp_mse_eval_batch(h, p(yd), rows, cols, cols, p(td), cols, p(wd), p(diff), cols) == 0
        aslp.check_error()
        st = (aslp.nnet.C.c_double * 3)()
        assert aslp.lib.aslp_mse_get_stats(h, st) != 0
        assert "not finite" in aslp.lib.aslp_nnet_last_error().decode()
        aslp.check_error()   # a host-side error: the device has none
        d = diff.cpu().numpy()
        assert np.isnan(d[3, 2]) and np.isfinite(np.delete(d.ravel(), 3 * cols + 2)).all()
    finally:
        aslp.lib.aslp_mse_free(h)
