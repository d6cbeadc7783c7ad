"""The per-timestep LSTM recurrence (csrc/rnn_fused.hip) at the recipes' size, with and without the split-fp16 products
(aslp_lstm_step_split16): one recurrent layer under an affine + softmax, train steps through the engine.

Per mode: ms per train step (wall, synchronised) and the recurrence alone -- the regions lstm_recurrence_fwd / lstm_recurrence_bwd of the
engine (device time between events around the T launches of a pass) -- as us per timestep, forward + backward.  The modes run as windows
in the order off / two pieces / off / one piece / off, `rounds` times over, in one process; the spread of the off windows is the noise floor.
Usage: python devtools/bench_lstm_step.py [rounds] [steps per window] [only: lstm | blstm]"""
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
A, D = 128, 512
# run_lstm.sh: cell_dim 1024, recurrent_dim 512, 64 streams of 40 frames; the BLSTM recipes: whole utterances, 20 streams of 400 frames
CASES = [("lstm", "LstmProjectedStreams", "<LstmProjectedStreams> <InputDim> %d <OutputDim> 512 <CellDim> 1024 <ParamScale> 0.02 <ClipGradient> 5.0" % D, 512, 64, 40),
         ("blstm", "BLstmProjectedStreams", "<BLstmProjectedStreams> <InputDim> %d <OutputDim> 1024 <CellDim> 1024 <ParamScale> 0.02 <ClipGradient> 5.0" % D, 1024, 20, 400)]
MODES = [("off", 0, 2), ("two pieces", 1, 2), ("off", 0, 2), ("one piece", 1, 1), ("off", 0, 2)]


def region(name):
    ms = C.c_double(0.0)
    n = aslp.lib.aslp_region_get(name.encode(), C.byref(ms))
    return int(n), ms.value


for key, name, line, od, S, T in CASES:
    if ONLY and ONLY != key:
        continue
    proto = "<NnetProto>\n%s\n<AffineTransform> <InputDim> %d <OutputDim> %d <BiasMean> 0.0 <BiasRange> 0.0 <ParamStddev> 0.04\n<Softmax> <InputDim> %d <OutputDim> %d\n</NnetProto>\n" % (line, od, A, A, A)
    net = aslp.Nnet.Init(proto, seed=1)
    net.SetTrainOptions(learn_rate=1e-5, momentum=0.9)
    xent = aslp.Xent()
    x = torch.randn(T * S, D, device=dev)
    lab = torch.randint(0, A, (T * S,), device=dev, dtype=torch.int32)
    net.SetSeqLengths([T] * S)
    count = [0]

    def step():
        net.ResetLstmStreams([1] * S if count[0] == 0 else [0] * S)
        net.TrainStepXent(xent, x, lab)
        count[0] += 1

    print("== %s C=1024 R=512 S=%d T=%d, %d steps per window" % (name, S, T, STEPS), flush=True)
    for r in range(ROUNDS):
        for label, on, pieces in MODES:
            aslp.ops.set_lstm_step_split16(on)
            aslp.ops.set_lstm_operand_pieces(pieces)
            step()   # warm-up of the mode (planes, scratch)
            assert aslp.lib.aslp_recurrent_last_path(0) == 2 and aslp.lib.aslp_recurrent_last_path(1) == 2, "not on the per-timestep path"
            assert aslp.lib.aslp_lstm_step_last_pieces() == (pieces if on else 0)
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
            (nf, fwd), (nb, bwd) = region("lstm_recurrence_fwd"), region("lstm_recurrence_bwd")
            aslp.lib.aslp_region_reset()
            print("round %d  %-10s  %8.3f ms/step   recurrence fwd %7.2f + bwd %7.2f = %7.2f us per timestep" %
                  (r, label, wall * 1e3, fwd / max(nf, 1) * 1e3 / T, bwd / max(nb, 1) * 1e3 / T, (fwd / max(nf, 1) + bwd / max(nb, 1)) * 1e3 / T), flush=True)
    aslp.ops.set_lstm_step_split16(-1)
    aslp.ops.set_lstm_operand_pieces(-1)
