"""CTC token errors: the host loop against the device kernel (csrc/ctc_errors.hip), in one process, host / device / host.
  (1) WarpCtc::ErrorRate alone on crafted activations: S = 32, A = 128, R = 200, T = 800, H = 50 / 200 / 400 / 800.  Per batch: the time
      the call keeps the host (wall clock around the call), the device time from its first launch to its last copy (events on the launch
      stream) and, for the device path, the wall clock until the book is settled.
  (2) The step loop Propagate -> Eval -> ErrorRate -> Backpropagate of the whole-utterance Warp-CTC configuration of bench.py's cfg3
      block (4 x BLstmProjectedStreamsLC + Affine 512 -> 128, S = 32, T in U(200, 800), L = T / 4), with the hypothesis lengths the
      net actually produced.
Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import aslp_import  # noqa: E402
import ctc_errors_ref as ref  # noqa: E402

aslp = aslp_import.load()
aslp.ops.use_torch_stream()
dev = torch.device("cuda:0")
S, A, R, T = 32, 128, 200, 800
ORDER = (("host_a", 1), ("device", 0), ("host_b", 1))


def error_rate_alone(H, reps=20):
    rng = np.random.default_rng(H)
    acts = np.zeros((T, S, A), np.float32)
    labels = []
    for s in range(S):
        hyp = [int(rng.integers(1, A))]
        while len(hyp) < H:   # no equal neighbours, so H = T needs no blank between them
            v = int(rng.integers(1, A))
            if v != hyp[-1]:
                hyp.append(v)
        acts[:, s] = ref.one_hot(ref.path_for(hyp, T, rng), A)
        labels.append([int(v) for v in rng.integers(1, A, R)])
    x = torch.from_numpy(acts.reshape(T * S, A)).to(dev)
    lens = np.full(S, T, np.int32)
    out = {"H": H}
    for name, on_host in ORDER:
        aslp.ops.ctc_errors_on_host(on_host)
        ctc = aslp.WarpCtc()
        call, devms, settled = [], [], []
        for i in range(reps + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            ctc.ErrorRate(lens, x, labels)
            e1.record()
            t1 = time.perf_counter()
            ctc.GetStats()   # settles the device path
            t2 = time.perf_counter()
            torch.cuda.synchronize()
            if i >= 3:
                call.append((t1 - t0) * 1e3)
                settled.append((t2 - t0) * 1e3)
                devms.append(e0.elapsed_time(e1))
        assert aslp.lib.aslp_ctc_errors_last_path() == 1 - on_host
        st = ctc.GetStats()
        out[name] = {"call_blocks_host_ms": float(np.median(call)), "stream_ms": float(np.median(devms)),
                     "until_settled_ms": float(np.median(settled)), "error_tokens": st["error_tokens"]}
    assert out["host_a"]["error_tokens"] == out["device"]["error_tokens"] == out["host_b"]["error_tokens"]
    return out


def step_loop(steps=6, warm=2):
    lines, d = ["<NnetProto>"], 40
    for _ in range(4):
        lines.append("<BLstmProjectedStreamsLC> <InputDim> %d <OutputDim> 512 <CellDim> 512 <ParamScale> 0.02 <ClipGradient> 5.0" % d)
        d = 512
    lines.append("<AffineTransform> <InputDim> 512 <OutputDim> %d <BiasMean> 0.0 <BiasRange> 0.0 <ParamStddev> 0.04" % A)
    proto = "\n".join(lines + ["</NnetProto>"]) + "\n"
    rng = np.random.default_rng(99)
    lens = rng.integers(200, 801, S).astype(np.int32)
    lens[0] = 800
    Tm = int(lens.max())
    lab = [[int(v) for v in rng.integers(1, A, max(1, int(t) // 4))] for t in lens]
    g = torch.Generator(device=dev)
    g.manual_seed(4321)
    xc = torch.randn(Tm * S, 40, device=dev, generator=g)
    out = {"max_frames": Tm, "steps": steps}
    for name, on_host in ORDER:
        aslp.ops.ctc_errors_on_host(on_host)
        net = aslp.Nnet.Init(proto, seed=777)   # the same start for every run
        net.SetTrainOptions(learn_rate=1e-5 / float(lens.sum()), momentum=0.9)
        ctc = aslp.WarpCtc()
        for i in range(warm):
            net.ResetLstmStreams([1] * S)
            net.TrainStepWarpCtc(ctc, xc, lens, lab)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            net.ResetLstmStreams([1] * S)
            net.TrainStepWarpCtc(ctc, xc, lens, lab)
        torch.cuda.synchronize()
        el = (time.perf_counter() - t0) / steps
        st = ctc.GetStats()
        out[name] = {"ms_per_step": el * 1e3, "error_tokens": st["error_tokens"], "ref_tokens": st["ref_tokens"]}
        if name == "device":   # what the net emits at this point: the hypothesis lengths of one more forward pass
            net.ResetLstmStreams([1] * S)
            y = net.Propagate(xc)
            _, hyps = aslp.ops.ctc_token_errors(y, lab, lens)
            hl = [len(h) for h in hyps]
            out["hyp_len"] = {"min": min(hl), "median": float(np.median(hl)), "max": max(hl)}
        del net
    assert out["host_a"]["error_tokens"] == out["device"]["error_tokens"] == out["host_b"]["error_tokens"]
    out["device_not_slower_than_slower_host"] = out["device"]["ms_per_step"] <= max(out["host_a"]["ms_per_step"], out["host_b"]["ms_per_step"])
    return out


if __name__ == "__main__":
    res = {"error_rate_alone": [error_rate_alone(H) for H in (50, 200, 400, 800)]}
    if "--no-step" not in sys.argv:
        res["step_loop"] = step_loop()
    aslp.ops.ctc_errors_on_host(-1)
    print(json.dumps(res))
