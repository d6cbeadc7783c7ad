"""ReLU hidden layers on the GPU: the shapes of BASELINE.json's cfg1 / cfg2 with <ReLU> in place of <Sigmoid> (5 x 2048, 440 -> 3000;
minibatch 256, and 1024 without BatchNormalization) and the run_cfsmn_pre.sh init net (AffineTransform -> ReLU -> LinearTransform, 437-row
utterance).  One line per configuration: ms per training step (host clock around a window that ends in a device synchronise, 50 warm-up steps)
and how many Tanh / ReLU layers rode in a product's epilogue.  ASLP_FUSE_TANH_RELU=0 gives the separate-launch path (A/B switch).
Usage: python devtools/bench_relu_dnn.py [steps] [config ...]     configs: relu256 relu1024 cfsmn_pre (default: all)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import aslp_import  # noqa: E402

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 300
CONFIGS = sys.argv[2:] or ["relu256", "relu1024", "cfsmn_pre"]
aslp = aslp_import.load()
aslp.ops.use_torch_stream()
dev = torch.device("cuda:0")


def relu_dnn():
    lines, d = ["<NnetProto>"], 440
    for _ in range(5):
        lines.append("<AffineTransform> <InputDim> %d <OutputDim> 2048 <BiasMean> 0.0 <BiasRange> 0.1 <ParamStddev> 0.02" % d)
        lines.append("<ReLU> <InputDim> 2048 <OutputDim> 2048")
        d = 2048
    lines += ["<AffineTransform> <InputDim> 2048 <OutputDim> 3000 <BiasMean> 0.0 <BiasRange> 0.0 <ParamStddev> 0.02",
              "<Softmax> <InputDim> 3000 <OutputDim> 3000", "</NnetProto>"]
    return "\n".join(lines) + "\n", 440, 3000


def cfsmn_pre():
    # run_cfsmn_pre.sh's init net: 40-dimensional features spliced over 11 frames in front of <AffineTransform> <ReLU> <LinearTransform>
    lines = ["<NnetProto>",
             "<AffineTransform> <InputDim> 440 <OutputDim> 1024 <BiasMean> 0.0 <BiasRange> 0.1 <ParamStddev> 0.02 <MaxNorm> 20",
             "<ReLU> <InputDim> 1024 <OutputDim> 1024",
             "<LinearTransform> <InputDim> 1024 <OutputDim> 512 <ParamStddev> 0.1",
             "<AffineTransform> <InputDim> 512 <OutputDim> 3000 <BiasMean> 0.0 <BiasRange> 0.0 <ParamStddev> 0.02",
             "<Softmax> <InputDim> 3000 <OutputDim> 3000", "</NnetProto>"]
    return "\n".join(lines) + "\n", 440, 3000


def run(name, proto, rows, lr):
    text, din, dout = proto
    net = aslp.Nnet.Init(text, seed=777)
    net.SetTrainOptions(learn_rate=lr, momentum=0.0)
    xent = aslp.Xent()
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(rows, din, device=dev, generator=g)
    lab = torch.randint(0, dout, (rows,), device=dev, dtype=torch.int32, generator=g)
    for _ in range(50):
        net.TrainStepXent(xent, x, lab)
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(STEPS):
        net.TrainStepXent(xent, x, lab)
    torch.cuda.synchronize()
    dt = (time.time() - t0) / STEPS
    fused = net.LastFusedActivations() if hasattr(net, "LastFusedActivations") else -1
    print("%s rows %d: %.4f ms/step, %.0f frames/s, fused Tanh/ReLU layers %d" % (name, rows, dt * 1e3, rows / dt, fused), flush=True)


for c in CONFIGS:
    if c == "relu256":
        run(c, relu_dnn(), 256, 1e-6)
    elif c == "relu1024":
        run(c, relu_dnn(), 1024, 1e-6)
    elif c == "cfsmn_pre":
        run(c, cfsmn_pre(), 437, 1e-6)
    else:
        raise SystemExit("unknown configuration " + c)
