"""One MultiTaskLoss training step, 440 -> 3 x 1024 Sigmoid -> 3040, <BlockSoftmax> 3000:40, tasks xent,3000,1 and xent,40,0.3, minibatch
256 and 1024 (DESIGN "MultiTaskLoss in one device pass"): Nnet.train_step_multitask with the switch on (the BlockSoftmax left to
aslp_xent_blocks_eval) and off (ASLP_MULTITASK_FUSED=0: the component, a dense target matrix, per task Eval, Scale, copy, the component's
backward), nothing on the host.  The switch-off route runs the kernels the step was made of before the entry point existed.

Usage: python devtools/bench_multitask_step.py [--steps 400] [--warm 50] [--rounds 3]
Every measurement is a child process: WARM steps, then STEPS steps inside a host-clock window that ends in a device synchronise.  The two
switch positions alternate, `rounds` times over, so that drift of the machine hits both alike; printed: every sample, then per position
and minibatch the median and the spread (max - min), and the one-launch median relative to the op sequence's.

       python devtools/bench_multitask_step.py --one SWITCH MB [--steps N] [--warm N]
runs one such measurement in this process: the program to put behind a profiler for the launches and copies per step."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D_IN, HID, BLOCKS, WEIGHTS = 440, 1024, (3000, 40), (1.0, 0.3)
MBS = (256, 1024)


def proto():
    lines, d = ["<NnetProto>"], D_IN
    for _ in range(3):
        lines.append("<AffineTransform> <InputDim> %d <OutputDim> %d <BiasMean> 0.0 <BiasRange> 0.1 <ParamStddev> 0.02" % (d, HID))
        lines.append("<Sigmoid> <InputDim> %d <OutputDim> %d" % (HID, HID))
        d = HID
    out = sum(BLOCKS)
    lines += ["<AffineTransform> <InputDim> %d <OutputDim> %d <BiasMean> 0.0 <BiasRange> 0.0 <ParamStddev> 0.02" % (d, out),
              "<BlockSoftmax> <InputDim> %d <OutputDim> %d <BlockDims> %s" % (out, out, ":".join(str(b) for b in BLOCKS)), "</NnetProto>"]
    return "\n".join(lines) + "\n"


def one(switch, mb, warm, steps):
    import torch
    sys.path.insert(0, HERE)
    import aslp_import
    aslp = aslp_import.load()
    aslp.ops.use_torch_stream()
    aslp.ops.multitask_fused(switch)
    dev = torch.device("cuda:0")
    net = aslp.Nnet.Init(proto(), seed=777)
    net.SetTrainOptions(learn_rate=1e-6, momentum=0.0)
    loss = aslp.MultiTaskLoss("multitask," + ",".join("xent,%d,%g" % (b, w) for b, w in zip(BLOCKS, WEIGHTS)))
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(mb, D_IN, device=dev, generator=g)
    labels = torch.stack([torch.randint(0, b, (mb,), device=dev, generator=g) for b in BLOCKS], dim=1).to(torch.int32).contiguous()
    for _ in range(warm):
        net.train_step_multitask(loss, x, labels)
    torch.cuda.synchronize()
    reads = aslp.ops.device_to_host_syncs()
    t0 = time.perf_counter()
    for _ in range(steps):
        net.train_step_multitask(loss, x, labels)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    reads = (aslp.ops.device_to_host_syncs() - reads) / steps
    assert net.LastLossFold() == (2 if switch else 0)
    print("STEP %.6f (fold %d, %.2f waiting device-to-host reads per step, %s)" % (ms, net.LastLossFold(), reads, loss.Report().splitlines()[-1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warm", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--one", nargs=2, type=int, metavar=("SWITCH", "MB"))
    a = ap.parse_args()
    if a.one:
        one(a.one[0], a.one[1], a.warm, a.steps)
        return
    samples = {}
    for rnd in range(a.rounds):
        for switch in (1, 0):
            for mb in MBS:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(switch), str(mb), "--steps", str(a.steps), "--warm", str(a.warm)],
                                   capture_output=True, timeout=900)
                m = re.search(r"STEP (\S+)", p.stdout.decode())
                if p.returncode != 0 or not m:
                    raise SystemExit("train_step_multitask child failed:\n%s" % p.stderr.decode()[-2000:])
                samples.setdefault((switch, mb), []).append(float(m.group(1)))
                print("round %d switch %d mb %4d: %.4f ms/step" % (rnd, switch, mb, float(m.group(1))), flush=True)
    print("\n%-12s %5s %10s %10s %16s" % ("route", "mb", "median ms", "spread ms", "vs op sequence"))
    for mb in MBS:
        off = statistics.median(samples[0, mb])
        for switch, name in ((0, "op sequence"), (1, "one launch")):
            v = samples[switch, mb]
            print("%-12s %5d %10.4f %10.4f %+15.2f%%" % (name, mb, statistics.median(v), max(v) - min(v), (statistics.median(v) / off - 1) * 100))


if __name__ == "__main__":
    main()
