"""The training steps tests/test_mse_engine_gpu.py compares between the two settings of ASLP_MSE_FUSED (read once per process): run
in-process for the default and, by running this file, in a fresh child process for ASLP_MSE_FUSED=0.  `python mse_engine_steps.py OUT.npz`
writes every result of run_all()."""
import os
import sys

import numpy as np

SMALL = dict(rows=24, dims=(12, 16, 10), act="Sigmoid", seed=11)       # fp32 instruction products only
SPLIT16 = dict(rows=128, dims=(128, 256, 128), act="Sigmoid", seed=12)  # the output layer's products on the split-fp16 kernels
STEPS = 2


def proto(dims, act):
    d_in, hid, out = dims
    return ("<NnetProto>\n"
            "<AffineTransform> <InputDim> %d <OutputDim> %d <BiasMean> -0.5 <BiasRange> 1.0 <ParamStddev> 0.1\n"
            "<%s> <InputDim> %d <OutputDim> %d\n"
            "<AffineTransform> <InputDim> %d <OutputDim> %d <BiasMean> 0.0 <BiasRange> 0.0 <ParamStddev> 0.1\n"
            "</NnetProto>\n" % (d_in, hid, act, hid, hid, hid, out))


def batches(cfg):
    rng = np.random.default_rng(cfg["seed"])
    rows, (d_in, _, out) = cfg["rows"], cfg["dims"]
    res = []
    for _ in range(STEPS):
        w = rng.choice(np.array([0.0, 0.5, 1.0, 2.0], np.float32), rows).astype(np.float32)
        res.append((rng.standard_normal((rows, d_in)).astype(np.float32), rng.standard_normal((rows, out)).astype(np.float32), w))
    return res


def run(aslp, dev, cfg, composed):
    """STEPS training steps: Nnet.train_step_mse, or (composed) Propagate + Mse.Eval + Backpropagate by hand.  Returns (parameters after each
    step [STEPS x n], [frames, loss, num_tgt])"""
    import torch
    net = aslp.Nnet.Init(proto(cfg["dims"], cfg["act"]), seed=cfg["seed"])
    net.SetTrainOptions(learn_rate=0.01, momentum=0.5)
    mse = aslp.Mse()
    params = []
    for x, t, w in batches(cfg):
        xd, td, wd = torch.from_numpy(x).to(dev), torch.from_numpy(t).to(dev), torch.from_numpy(w).to(dev)
        if composed:
            y = net.Propagate(xd)
            diff = torch.empty_like(y)
            mse.Eval(wd, y, td, diff)
            net.Backpropagate(diff)
        else:
            net.train_step_mse(mse, xd, td, wd)
        params.append(net.GetParams().copy())
    st = mse.GetStats()
    return np.stack(params), np.array([st["frames"], st["loss"], st["num_tgt"]], np.float64)


def run_all(aslp, dev):
    out = {}
    for name, cfg, composed in (("small_step", SMALL, False), ("small_composed", SMALL, True), ("split16_step", SPLIT16, False)):
        p, s = run(aslp, dev, cfg, composed)
        out[name + "_params"], out[name + "_stats"] = p, s
    return out


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch
    import aslp_import
    pkg = aslp_import.load()
    pkg.ops.use_torch_stream()
    np.savez(sys.argv[1], **run_all(pkg, torch.device("cuda:0")))
