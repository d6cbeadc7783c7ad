"""The per-timestep GRU recurrence (csrc/gru_fused.hip) at the recipes' width, with and without the fp16-piece products
(aslp_gru_step_pieces): one GruStreams layer under an affine + softmax, train steps through the engine.

Per mode: ms per train step (wall, synchronised) and the recurrence alone -- the regions gru_recurrence_fwd / gru_recurrence_bwd of the
engine (device time between events around one pass: with pieces the conversion of the two weight matrices, then the T x 2 launches) -- as
us per timestep, forward + backward.  The modes run as windows in the order off / two pieces / off / one piece / off, `rounds` times over,
in one process; the off windows run the fp32-instruction kernels, and their spread is the noise floor.
Usage: python devtools/bench_gru_step.py [rounds] [steps per window] [only: s64 | s20]"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import aslp_import

aslp = aslp_import.load()
aslp.ops.use_torch_stream()
dev = torch.device("cuda:0")
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 2
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
ONLY = sys.argv[3] if len(sys.argv) > 3 else ""
A, D, H = 128, 512, 1024
# a GRU in the recipes' 1024-wide slot: 64 streams of 40 frames (run_lstm.sh's batch) and 20 streams of 400 frames (the BLSTM recipes')
CASES = [("s64", 64, 40), ("s20", 20, 400)]
MODES = [("off", 0), ("two pieces", 2), ("off", 0), ("one piece", 1), ("off", 0)]


def region(name):
    ms = C.c_double(0.0)
    n = aslp.lib.aslp_region_get(name.encode(), C.byref(ms))
    return int(n), ms.value


for key, S, T in CASES:
    if ONLY and ONLY != key:
        continue
    proto = ("<NnetProto>\n<GruStreams> <InputDim> %d <OutputDim> %d <ParamScale> 0.02 <ClipGradient> 5.0\n"
             "<AffineTransform> <InputDim> %d <OutputDim> %d <BiasMean> 0.0 <BiasRange> 0.0 <ParamStddev> 0.04\n<Softmax> <InputDim> %d <OutputDim> %d\n</NnetProto>\n"
             % (D, H, H, A, A, A))
    net = aslp.Nnet.Init(proto, seed=1)
    net.SetTrainOptions(learn_rate=1e-5, momentum=0.9)
    xent = aslp.Xent()
    x = torch.randn(T * S, D, device=dev)
    lab = torch.randint(0, A, (T * S,), device=dev, dtype=torch.int32)
    count = [0]

    def step():
        net.ResetLstmStreams([1] * S if count[0] == 0 else [0] * S)
        net.TrainStepXent(xent, x, lab)
        count[0] += 1

    print("== GruStreams H=%d S=%d T=%d, %d steps per window" % (H, S, T, STEPS), flush=True)
    for r in range(ROUNDS):
        for label, pieces in MODES:
            aslp.ops.set_gru_step_pieces(pieces)
            step()   # warm-up of the mode (planes)
            assert aslp.lib.aslp_recurrent_last_path(0) == 2 and aslp.lib.aslp_recurrent_last_path(1) == 2, "not on the per-timestep path"
            assert aslp.lib.aslp_gru_step_last_pieces() == pieces
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(STEPS):
                step()
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) / STEPS
            aslp.lib.aslp_region_reset()
            aslp.lib.aslp_region_profile(1)
            for _ in range(STEPS):
                step()
            torch.cuda.synchronize()
            aslp.lib.aslp_region_profile(0)
            (nf, fwd), (nb, bwd) = region("gru_recurrence_fwd"), region("gru_recurrence_bwd")
            aslp.lib.aslp_region_reset()
            print("round %d  %-10s  %8.3f ms/step   recurrence fwd %7.2f + bwd %7.2f = %7.2f us per timestep" %
                  (r, label, wall * 1e3, fwd / max(nf, 1) * 1e3 / T, bwd / max(nb, 1) * 1e3 / T, (fwd / max(nf, 1) + bwd / max(nb, 1)) * 1e3 / T), flush=True)
    aslp.ops.set_gru_step_pieces(-1)
