"""MultiTaskLoss through the engine: nnet.MultiTaskLoss and the C ABI under it (aslp_multitask_*), Nnet.train_step_multitask with the final
<BlockSoftmax> left to the loss kernel, the nets where it cannot be, and the A/B switch (ops.multitask_fused) that gives the op sequence
of MultiTaskLoss::Eval back.  Three steps with momentum 0.5 and learn rate 0.02 against the oracle chain (oracle.Affine, orc_sigmoid, the
block softmax of tests/multitask_ref.py rounded to fp32, oracle.multitask_eval, BlockSoftmax' backward mask) at the bars of
tests/test_multitask_gpu.py: 1e-4 on the parameters, 2e-4 on the gradient applied per tensor."""
import re

import numpy as np
import pytest
import torch

import multitask_ref as ref
import nnet_io

pytestmark = pytest.mark.gpu
LR, MOM, STEPS = 0.02, 0.5, 3

# name: input, hidden, output layer's widths; what follows the output layer; the loss' tasks; minibatch; the fold expected
CONFIGS = {
    "folded": dict(dims=(12, 24, 16), out=("block", [10, 6]), spec=[("xent", 10, 1.0), ("xent", 6, 0.25)], mb=16, fold=2),
    "medium_narrow": dict(dims=(12, 32, 556), out=("block", [516, 40]), spec=[("xent", 516, 1.0), ("xent", 40, 0.25)], mb=8, fold=2),
    "other_blocks": dict(dims=(12, 24, 16), out=("block", [8, 8]), spec=[("xent", 10, 1.0), ("xent", 6, 0.25)], mb=16, fold=0),
    "sigmoid_mse": dict(dims=(12, 24, 16), out=("sigmoid", None), spec=[("xent", 10, 1.0), ("mse", 6, 0.25)], mb=16, fold=0),
}


def spec_string(spec):
    return "multitask," + ",".join("%s,%d,%g" % t for t in spec)


def task_blocks(spec):
    out, o = [], 0
    for _, d, _ in spec:
        out.append((o, d))
        o += d
    return out


def make(cfg, seed):
    """initial parameters and the minibatches: x, labels [mb x xent tasks] (some -1), dense targets (the mse windows filled), weights"""
    rng = np.random.default_rng(seed)
    D, H, O = cfg["dims"]
    W1, b1 = rng.standard_normal((H, D)).astype(np.float32) * 0.3, rng.standard_normal(H).astype(np.float32) * 0.1
    W2, b2 = rng.standard_normal((O, H)).astype(np.float32) * 0.3, rng.standard_normal(O).astype(np.float32) * 0.1
    mb, spec = cfg["mb"], cfg["spec"]
    xent = [(o, d) for (o, d), (k, _, _) in zip(task_blocks(spec), spec) if k == "xent"]
    batches = []
    for s in range(STEPS):
        x = rng.standard_normal((mb, D)).astype(np.float32)
        labels = np.stack([rng.integers(0, d, mb) for _, d in xent], axis=1).astype(np.int32)
        labels[(1 + s) % mb, 0] = -1
        labels[(5 + s) % mb, -1] = -1
        tgt = ref.dense_targets(xent, labels, O)
        for (o, d), (k, _, _) in zip(task_blocks(spec), spec):
            if k == "mse":
                tgt[:, o:o + d] = rng.uniform(0.05, 0.95, (mb, d)).astype(np.float32)
        fw = rng.choice(np.array([0.0, 1.0, 1.0, 2.0], np.float32), mb)
        batches.append((x, labels, tgt, fw))
    return (W1, b1, W2, b2), batches


def write_net(path, cfg, params):
    D, H, O = cfg["dims"]
    W1, b1, W2, b2 = params
    kind, dims = cfg["out"]
    last = ("<BlockSoftmax>", O, O, nnet_io.ivec(dims)) if kind == "block" else ("<Sigmoid>", O, O, b"")
    nnet_io.write_simple_nnet(path, [("<AffineTransform>", D, H, nnet_io.affine(W1, b1)), ("<Sigmoid>", H, H, b""),
                                     ("<AffineTransform>", H, O, nnet_io.affine(W2, b2)), last])


def run_engine(aslp, dev, cfg, params, batches, path):
    """three train_step_multitask calls from `params`; the parameters after the last, the fold of every step, per-task stats, Report()"""
    write_net(path, cfg, params)
    net = aslp.Nnet.Read(path)
    net.SetTrainOptions(learn_rate=LR, momentum=MOM)
    loss = aslp.MultiTaskLoss(spec_string(cfg["spec"]))
    assert loss.NumTasks() == len(cfg["spec"])
    has_mse = any(k == "mse" for k, _, _ in cfg["spec"])
    folds = []
    for x, labels, tgt, fw in batches:
        net.train_step_multitask(loss, torch.from_numpy(x).to(dev), torch.from_numpy(labels).to(dev),
                                 torch.from_numpy(tgt).to(dev) if has_mse else None, torch.from_numpy(fw).to(dev))
        folds.append(net.LastLossFold())
    return dict(params=net.GetParams(), folds=folds, stats=[loss.GetStats(i) for i in range(loss.NumTasks())], report=loss.Report(),
                avg=loss.AvgLoss(), net=net)


def run_oracle(oracle, cfg, params, batches):
    W1, b1, W2, b2 = params
    A1, A2 = oracle.Affine(W1, b1), oracle.Affine(W2, b2)
    kind, dims = cfg["out"]
    spec = cfg["spec"]
    stats = [dict(frames=0.0, correct=0.0, loss=0.0, entropy=0.0, likelyhood=0.0) if k == "xent" else dict(loss=0.0, frames=0.0) for k, _, _ in spec]
    for x, labels, tgt, fw in batches:
        h = oracle.unary("orc_sigmoid", A1.propagate(x))
        a = A2.propagate(h)
        if kind == "block":
            blocks = task_blocks([("xent", d, 1.0) for d in dims])
            p = ref.block_softmax(a, blocks)
            for o, d in blocks:
                assert (ref.argmax_gap(p[:, o:o + d]) > ref.ARGMAX_GAP).all()   # no rounding decides `correct`
            y = p.astype(np.float32)
        else:
            y = oracle.unary("orc_sigmoid", a)
        diff, st = oracle.multitask_eval(spec, fw, y, tgt)
        for acc, inc in zip(stats, st):
            for k in acc:
                acc[k] += inc[k]
        if kind == "block":   # BlockSoftmax::BackpropagateFnc: every block's row times (1 - its sum)
            d2 = np.array(diff, np.float64)
            for o, d in blocks:
                d2[:, o:o + d] *= 1.0 - d2[:, o:o + d].sum(axis=1, keepdims=True)
            d2 = d2.astype(np.float32)
        else:
            d2 = oracle.binary("orc_diff_sigmoid", y, diff)
        dh = A2.backpropagate(d2)
        A2.update(h, d2, LR, MOM)
        d1 = oracle.binary("orc_diff_sigmoid", h, dh)
        A1.update(x, d1, LR, MOM)
    return dict(params=np.concatenate([A1.W.ravel(), A1.b, A2.W.ravel(), A2.b]), stats=stats)


def per_tensor(params):
    return [(o, o + t.size) for o, t in zip(np.cumsum([0] + [p.size for p in params[:-1]]), params)]


def check_against_oracle(oracle, cfg, params, got, want):
    init = np.concatenate([p.ravel() for p in params])
    assert got["params"].shape == want["params"].shape and np.isfinite(got["params"]).all()
    print("parameters rel err %.3g" % oracle.rel_err(got["params"], want["params"]))
    assert oracle.rel_err(got["params"], want["params"]) < 1e-4
    for lo, hi in per_tensor(params):   # the gradient actually applied over the run, per tensor
        err = oracle.rel_err(got["params"][lo:hi] - init[lo:hi], want["params"][lo:hi] - init[lo:hi])
        print("applied gradient [%d:%d] rel err %.3g" % (lo, hi, err))
        assert err < 2e-4, (lo, hi)
    close = lambda a, b: abs(a - b) <= 2e-4 * max(abs(b), 1e-3)
    for (k, _, _), g, w in zip(cfg["spec"], got["stats"], want["stats"]):
        assert g["kind"] == k and g["frames"] == w["frames"]
        if k == "xent":
            assert g["correct"] == w["correct"]
            assert close(g["loss"], w["loss"]) and close(g["entropy"], w["entropy"]) and close(g["likelyhood"], w["likelyhood"])
        else:
            assert close(g["loss"], w["loss"])


@pytest.mark.parametrize("name", ["folded", "medium_narrow"])
def test_block_softmax_left_to_the_loss(aslp, oracle, dev, tmp_path, name):
    cfg = CONFIGS[name]
    params, batches = make(cfg, 300 + len(name))
    got = run_engine(aslp, dev, cfg, params, batches, tmp_path / "m.nnet")
    assert got["folds"] == [2] * STEPS
    check_against_oracle(oracle, cfg, params, got, run_oracle(oracle, cfg, params, batches))
    # the folded component's output was never made
    n = got["net"].NumComponents()
    with pytest.raises(RuntimeError, match="not materialised"):
        got["net"].ComponentOutput(n - 1, cfg["mb"], cfg["dims"][2])
    # Report(), nnet-loss.cc:370-393, with the values GetStats gives (the regular expression of tests/test_multitask_gpu.py, two Xent tasks)
    m = re.fullmatch(r"MultiTaskLoss, with 2 parallel loss functions\.\n"
                     r"Loss 1, AvgLoss: (\S+) \(Xent\), Likelyhood: (\S+) Frame: (\S+)\nFRAME_ACCURACY >> (\S+)% <<\n\n"
                     r"Loss 2, AvgLoss: (\S+) \(Xent\), Likelyhood: (\S+) Frame: (\S+)\nFRAME_ACCURACY >> (\S+)% <<\n\n"
                     r"Loss \(OVERALL\), AvgLoss: (\S+) \(MultiTaskLoss\), weights (\S+) (\S+) , values (\S+) (\S+) \n", got["report"])
    assert m, got["report"]
    v = [float(x) for x in m.groups()]
    close = lambda a, b: abs(a - b) <= 2e-5 * max(abs(b), 1e-3)   # (six printed digits)
    avgs = []
    for i, st in enumerate(got["stats"]):
        avg = (st["loss"] - st["entropy"]) / st["frames"]
        avgs.append(avg)
        assert close(v[4 * i], avg) and close(v[4 * i + 1], st["likelyhood"] / st["frames"]) and v[4 * i + 2] == st["frames"]
        assert close(v[4 * i + 3], 100.0 * st["correct"] / st["frames"])
    w1, w2 = cfg["spec"][0][2], cfg["spec"][1][2]
    overall = np.float32(w1) * np.float32(avgs[0]) + np.float32(w2) * np.float32(avgs[1])
    assert close(v[8], overall) and m.group(10) == "%g" % w1 and m.group(11) == "%g" % w2 and close(v[11], avgs[0]) and close(v[12], avgs[1])
    assert close(got["avg"], overall)


@pytest.mark.parametrize("name", ["other_blocks", "sigmoid_mse"])
def test_not_foldable_still_right(aslp, oracle, dev, tmp_path, name):
    """block dims that are not the task dims, and a Sigmoid output with an mse task: the component and its backward run as components"""
    cfg = CONFIGS[name]
    params, batches = make(cfg, 400 + len(name))
    got = run_engine(aslp, dev, cfg, params, batches, tmp_path / "m.nnet")
    assert got["folds"] == [0] * STEPS
    check_against_oracle(oracle, cfg, params, got, run_oracle(oracle, cfg, params, batches))
    n = got["net"].NumComponents()
    assert got["net"].ComponentOutput(n - 1, cfg["mb"], cfg["dims"][2]).shape == (cfg["mb"], cfg["dims"][2])


@pytest.mark.parametrize("name", ["folded", "medium_narrow", "sigmoid_mse"])
def test_switch_on_against_switch_off(aslp, dev, tmp_path, name):
    """same process, same inputs: the one-launch route against today's op sequence (no fold, a dense target matrix from the labels, per
    task Eval, Scale, copy, the component's backward).  2e-6 relative l2 per tensor, the bar tests/test_mse_engine_gpu.py holds its two
    modes to: the two routes differ in the order of the mask's fp32 row sum alone."""
    cfg = CONFIGS[name]
    params, batches = make(cfg, 500 + len(name))
    on = run_engine(aslp, dev, cfg, params, batches, tmp_path / "on.nnet")
    aslp.ops.multitask_fused(0)
    try:
        off = run_engine(aslp, dev, cfg, params, batches, tmp_path / "off.nnet")
    finally:
        aslp.ops.multitask_fused(1)
    assert on["folds"] == [cfg["fold"]] * STEPS and off["folds"] == [0] * STEPS
    for a, b in zip(on["stats"], off["stats"]):
        assert a["frames"] == b["frames"] and a["kind"] == b["kind"]
        if a["kind"] == "xent":
            assert a["correct"] == b["correct"]
        assert abs(a["loss"] - b["loss"]) <= 1e-5 * abs(b["loss"]) + 1e-6
    assert not np.array_equal(on["params"], np.concatenate([p.ravel() for p in params]))
    worst = 0.0
    for lo, hi in per_tensor(params):
        ta, tb = on["params"][lo:hi].astype(np.float64), off["params"][lo:hi].astype(np.float64)
        worst = max(worst, float(np.linalg.norm(ta - tb) / np.linalg.norm(tb)))
    print("%s: worst per-tensor distance between the routes %.3g" % (name, worst))
    for lo, hi in per_tensor(params):
        ta, tb = on["params"][lo:hi].astype(np.float64), off["params"][lo:hi].astype(np.float64)
        assert np.linalg.norm(ta - tb) <= 2e-6 * np.linalg.norm(tb), (lo, hi)


def test_eval_batch_matches_kernel_reference(aslp, dev):
    """nnet.MultiTaskLoss.Eval on posteriors (nothing folded): xent windows as aslp_xent_eval x the task weight, bit for bit, on both routes"""
    spec = [("xent", 10, 1.0), ("xent", 6, 0.25)]
    rng = np.random.default_rng(8)
    rows = 9
    blocks = task_blocks(spec)
    post = ref.block_softmax(np.concatenate([ref.safe_logits(rng, rows, d) for _, d in blocks], axis=1), blocks).astype(np.float32)
    labels = np.stack([rng.integers(0, d, rows) for _, d in blocks], axis=1).astype(np.int32)
    labels[2, 0], labels[4, 1] = -1, -1
    fw = np.array([0, 1, 2] * 3, np.float32)
    pd, ld, fd = torch.from_numpy(post).to(dev), torch.from_numpy(labels).to(dev), torch.from_numpy(fw).to(dev)
    want = np.empty_like(post)
    for b, ((o, d), (_, _, w)) in enumerate(zip(blocks, spec)):
        dd = torch.empty((rows, d), dtype=torch.float32, device=dev)
        aslp.ops.xent_eval(pd[:, o:o + d], fd, dd, torch.zeros(5, dtype=torch.float64, device=dev), labels=ld[:, b].contiguous())
        want[:, o:o + d] = (dd * np.float32(w)).cpu().numpy()
    _, stats = ref.model(post, blocks, [1.0, 0.25], labels, fw, mask=False)
    for mode in (1, 0):
        aslp.ops.multitask_fused(mode)
        try:
            loss = aslp.MultiTaskLoss(spec_string(spec))
            diff = torch.full_like(pd, -5.0)
            loss.Eval(fd, pd, diff, labels=ld)
            assert np.array_equal(diff.cpu().numpy().view(np.uint32), want.view(np.uint32)), mode
            for i, st in enumerate(stats):
                g = loss.GetStats(i)
                assert g["frames"] == st["frames"] and g["correct"] == st["correct"] and abs(g["loss"] - st["loss"]) <= 1e-5 * st["loss"]
            # frame_weights None: ones
            loss.Eval(None, pd, diff, labels=ld)
            assert loss.GetStats(0)["frames"] == stats[0]["frames"] + (labels[:, 0] >= 0).sum()
        finally:
            aslp.ops.multitask_fused(1)


def test_errors(aslp, dev):
    C = aslp.nnet.C
    h = aslp.nnet._H()
    assert aslp.lib.aslp_multitask_create(b"multitask,xent,10", C.byref(h)) != 0      # not triplets (nnet-loss.cc:300)
    assert aslp.lib.aslp_nnet_last_error().decode() != ""
    with pytest.raises(RuntimeError):
        aslp.MultiTaskLoss("multitask,ctc,10,1.0")
    with pytest.raises(RuntimeError):
        aslp.MultiTaskLoss("")
    y = torch.zeros((4, 17), dtype=torch.float32, device=dev)
    lab = torch.zeros((4, 2), dtype=torch.int32, device=dev)
    loss = aslp.MultiTaskLoss("multitask,xent,10,1.0,xent,6,0.25")
    with pytest.raises(RuntimeError, match="17 columns"):       # cols differ from the task dims' sum
        loss.Eval(None, y, torch.empty_like(y), labels=lab)
    mixed = aslp.MultiTaskLoss("multitask,xent,10,1.0,mse,6,0.25")
    y16 = torch.full((4, 16), 0.5, dtype=torch.float32, device=dev)
    with pytest.raises(RuntimeError, match="dense targets"):    # an mse task without targets
        mixed.Eval(None, y16, torch.empty_like(y16), labels=lab[:, :1].contiguous())
    aslp.check_error()
