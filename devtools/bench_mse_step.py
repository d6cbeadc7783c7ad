"""One Mse training step, 440 -> 3 x 2048 ReLU -> 257 linear, minibatch 256 and 1024, in one or several builds of this repository side
by side (DESIGN "Mse in one device pass").

Two forms of the step:
  tool   aslp-nnet-train-mse of the build on synthetic tables: Propagate / Mse::Eval / Backpropagate as the tools compose them, file
         reading and the randomizers included.  Every build has it.  Two runs, WARM and WARM + STEPS minibatches long; the step is the
         difference of the tool's own elapsed times (its "fps" line) over STEPS.  The tables are one 4096-frame utterance in an archive
         and a script file that names it once per utterance needed, so the files stay small.
  step   Nnet.train_step_mse from Python, nothing on the host: WARM steps, then STEPS steps inside a host-clock window that ends in a
         device synchronise.  Only builds that have the entry point.

Usage: python devtools/bench_mse_step.py [--steps 400] [--warm 50] [--rounds 3] [--tmp DIR] NAME=TREE[,ENV=VALUE...] ...
e.g.   python devtools/bench_mse_step.py parent=/path/to/parent new=. ops=.,ASLP_MSE_FUSED=0
The builds are measured in the order given, `rounds` times over (alternating, so that drift of the machine hits all of them alike);
printed: every sample, then per build and configuration the median and the spread (max - min), each build's median relative to the
first build's, and whether it lies inside the first build's own spread."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tests"))
import kaldi_formats as kf  # noqa: E402

D_IN, HID, D_OUT, UTT = 440, 2048, 257, 4096
MBS = (256, 1024)


def proto():
    lines, d = ["<NnetProto>"], D_IN
    for _ in range(3):
        lines.append("<AffineTransform> <InputDim> %d <OutputDim> %d <BiasMean> 0.0 <BiasRange> 0.1 <ParamStddev> 0.02" % (d, HID))
        lines.append("<ReLU> <InputDim> %d <OutputDim> %d" % (HID, HID))
        d = HID
    lines += ["<AffineTransform> <InputDim> %d <OutputDim> %d <BiasMean> 0.0 <BiasRange> 0.0 <ParamStddev> 0.02" % (d, D_OUT), "</NnetProto>"]
    return "\n".join(lines) + "\n"


STEP_CHILD = r'''
import sys, time
import torch
sys.path.insert(0, sys.argv[1])
import aslp_import
aslp = aslp_import.load(); aslp.ops.use_torch_stream()
if not hasattr(aslp.Nnet, "train_step_mse"):
    print("STEP none"); sys.exit(0)
mb, warm, steps = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
dev = torch.device("cuda:0")
net = aslp.Nnet.Init(open(sys.argv[5]).read(), seed=777)
net.SetTrainOptions(learn_rate=1e-6, momentum=0.0)
mse = aslp.Mse()
g = torch.Generator(device=dev).manual_seed(5)
x = torch.randn(mb, net.InputDim(), device=dev, generator=g)
t = torch.randn(mb, net.OutputDim(), device=dev, generator=g)
for _ in range(warm):
    net.train_step_mse(mse, x, t)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(steps):
    net.train_step_mse(mse, x, t)
torch.cuda.synchronize()
print("STEP %.6f" % ((time.perf_counter() - t0) / steps * 1e3))
'''


def write_tables(tmp):
    rng = np.random.default_rng(0)
    for name, cols in (("feats", D_IN), ("tgts", D_OUT)):
        with open(os.path.join(tmp, name + ".ark"), "wb") as f:
            f.write(b"u " + kf.matrix_bin(rng.standard_normal((UTT, cols), dtype=np.float32)))
    open(os.path.join(tmp, "nnet.proto"), "w").write(proto())


def write_scripts(tmp, tag, n_utt):
    for name in ("feats", "tgts"):
        with open(os.path.join(tmp, "%s_%s.scp" % (name, tag)), "w") as f:
            for i in range(n_utt):
                f.write("utt%05d %s:2\n" % (i, os.path.join(tmp, name + ".ark")))   # (2: behind the key "u " of the archive's one entry)


def tool_elapsed(tree, env, tmp, tag, mb, n_utt):
    exe = os.path.join(tree, "kaldi-aslp_amd", "bin", "aslp-nnet-train-mse")
    p = subprocess.run([exe, "--print-args=false", "--learn-rate=0.000001", "--minibatch-size=%d" % mb, "--randomizer-size=32768",
                        "scp:%s/feats_%s.scp" % (tmp, tag), "scp:%s/tgts_%s.scp" % (tmp, tag), tmp + "/nnet.init", tmp + "/nnet.out"],
                       env=env, capture_output=True, timeout=900)
    err = p.stderr.decode()
    m = re.search(r"min, fps([0-9.eE+-]+)\]", err)
    if p.returncode != 0 or not m:
        raise SystemExit("aslp-nnet-train-mse failed in %s:\n%s" % (tree, err[-2000:]))
    return n_utt * UTT / float(m.group(1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warm", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("builds", nargs="+")
    a = ap.parse_args()
    builds = []
    for b in a.builds:
        name, rest = b.split("=", 1)
        parts = rest.split(",")
        builds.append((name, os.path.abspath(parts[0]), dict(kv.split("=", 1) for kv in parts[1:])))
    tmp = a.tmp or tempfile.mkdtemp(prefix="mse_step_")
    os.makedirs(tmp, exist_ok=True)
    write_tables(tmp)
    subprocess.run([os.path.join(builds[0][1], "kaldi-aslp_amd", "bin", "aslp-nnet-init"), "--print-args=false", "--seed=777", tmp + "/nnet.proto",
                    tmp + "/nnet.init"], check=True, capture_output=True)
    utts = {}
    for mb in MBS:
        per = UTT // mb   # minibatches per utterance
        utts[mb] = ((a.warm + per - 1) // per, (a.warm + a.steps + per - 1) // per)
        write_scripts(tmp, "warm%d" % mb, utts[mb][0])
        write_scripts(tmp, "full%d" % mb, utts[mb][1])
    samples = {}
    for rnd in range(a.rounds):
        for name, tree, extra in builds:
            env = dict(os.environ, **extra)
            for mb in MBS:
                n_w, n_f = utts[mb]
                t_w = tool_elapsed(tree, env, tmp, "warm%d" % mb, mb, n_w)
                t_f = tool_elapsed(tree, env, tmp, "full%d" % mb, mb, n_f)
                ms = (t_f - t_w) / ((n_f - n_w) * (UTT // mb)) * 1e3
                samples.setdefault((name, "tool", mb), []).append(ms)
                print("round %d %-8s tool mb %4d: %.4f ms/step" % (rnd, name, mb, ms), flush=True)
                p = subprocess.run([sys.executable, "-c", STEP_CHILD, tree, str(mb), str(a.warm), str(a.steps), tmp + "/nnet.proto"], env=env,
                                   capture_output=True, timeout=900)
                m = re.search(r"STEP (\S+)", p.stdout.decode())
                if p.returncode != 0 or not m:
                    raise SystemExit("train_step_mse child failed in %s:\n%s" % (tree, p.stderr.decode()[-2000:]))
                if m.group(1) != "none":
                    samples.setdefault((name, "step", mb), []).append(float(m.group(1)))
                    print("round %d %-8s step mb %4d: %.4f ms/step" % (rnd, name, mb, float(m.group(1))), flush=True)
    first = builds[0][0]
    print("\n%-8s %-5s %5s %10s %10s %12s  %s" % ("build", "form", "mb", "median ms", "spread ms", "vs " + first, "inside its spread"))
    for (name, form, mb), v in sorted(samples.items(), key=lambda kv: (kv[0][1], kv[0][2], [b[0] for b in builds].index(kv[0][0]))):
        med, spread = statistics.median(v), max(v) - min(v)
        ref = samples.get((first, form, mb))
        if ref:
            rmed, rspread = statistics.median(ref), max(ref) - min(ref)
            print("%-8s %-5s %5d %10.4f %10.4f %+11.2f%%  %s" % (name, form, mb, med, spread, (med / rmed - 1) * 100, "yes" if med <= rmed + rspread else "NO"))
        else:
            print("%-8s %-5s %5d %10.4f %10.4f %12s  -" % (name, form, mb, med, spread, "-"))


if __name__ == "__main__":
    main()
