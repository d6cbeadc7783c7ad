"""One Xent training step on soft targets, 440 -> 3 x 2048 Sigmoid -> 3000 Softmax, three (pdf, weight) pairs per frame, minibatch 256 and
1024, in one or several builds of this repository side by side (DESIGN "Soft targets in one device pass").

Two forms of the step:
  tool   aslp-nnet-train-frame of the build on synthetic tables: Propagate / Xent::EvalOnLossInput(Posterior) / Backpropagate as the tool
         composes them, file reading and the randomizer included.  Every build has it.  Two runs, WARM and WARM + STEPS minibatches long;
         the step is the difference of the tool's own elapsed times (its "fps" line) over STEPS.  The tables are one 4096-frame utterance
         in an archive and a script file that names it once per utterance needed, so the files stay small.
  step   from Python, nothing on the host: Nnet.train_step_xent_sparse where the build has it, else what a user of that build had to
         compose -- Propagate, Xent.Eval(targets=<dense matrix>), Backpropagate (printed as "step*").  WARM steps, then STEPS steps inside
         a host-clock window that ends in a device synchronise.

Usage: python devtools/bench_xent_soft_step.py [--steps 400] [--warm 50] [--rounds 3] [--tmp DIR] NAME=TREE[,ENV=VALUE...] ...
e.g.   python devtools/bench_xent_soft_step.py parent=/path/to/parent new=. dense=.,ASLP_XENT_SPARSE=0
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

D_IN, HID, D_OUT, UTT, NNZ = 440, 2048, 3000, 4096, 3
MBS = (256, 1024)


def proto():
    lines, d = ["<NnetProto>"], D_IN
    for _ in range(3):
        lines.append("<AffineTransform> <InputDim> %d <OutputDim> %d <BiasMean> 0.0 <BiasRange> 0.1 <ParamStddev> 0.02" % (d, HID))
        lines.append("<Sigmoid> <InputDim> %d <OutputDim> %d" % (HID, HID))
        d = HID
    lines += ["<AffineTransform> <InputDim> %d <OutputDim> %d <BiasMean> 0.0 <BiasRange> 0.0 <ParamStddev> 0.02" % (d, D_OUT),
              "<Softmax> <InputDim> %d <OutputDim> %d" % (D_OUT, D_OUT), "</NnetProto>"]
    return "\n".join(lines) + "\n"


STEP_CHILD = r'''
import sys, time
import torch
sys.path.insert(0, sys.argv[1])
import aslp_import
aslp = aslp_import.load(); aslp.ops.use_torch_stream()
mb, warm, steps = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
dev = torch.device("cuda:0")
net = aslp.Nnet.Init(open(sys.argv[5]).read(), seed=777)
net.SetTrainOptions(learn_rate=1e-6, momentum=0.0)
xent = aslp.Xent()
g = torch.Generator(device=dev).manual_seed(5)
x = torch.randn(mb, net.InputDim(), device=dev, generator=g)
cols = net.OutputDim()
pdf = torch.stack([torch.randperm(cols, device=dev, generator=g)[:3].sort().values for _ in range(mb)]).to(torch.int32)
w = torch.tensor([0.5, 0.375, 0.125], device=dev).repeat(mb)
fw = torch.ones(mb, device=dev)
if hasattr(aslp.Nnet, "train_step_xent_sparse"):
    form = "step"
    rb = torch.arange(0, 3 * mb + 1, 3, dtype=torch.int32, device=dev)
    c = pdf.reshape(-1).contiguous()
    step = lambda: net.train_step_xent_sparse(xent, x, rb, c, w, fw)
else:
    form = "step*"
    tgt = torch.zeros(mb, cols, device=dev)
    tgt.scatter_(1, pdf.long(), w.view(mb, 3))
    diff = torch.empty(mb, cols, device=dev)
    def step():
        y = net.Propagate(x)
        xent.Eval(fw, y, diff, targets=tgt)
        net.Backpropagate(diff)
for _ in range(warm):
    step()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(steps):
    step()
torch.cuda.synchronize()
print("STEP %s %.6f" % (form, (time.perf_counter() - t0) / steps * 1e3))
'''


def write_tables(tmp):
    rng = np.random.default_rng(0)
    with open(os.path.join(tmp, "feats.ark"), "wb") as f:
        f.write(b"u " + kf.matrix_bin(rng.standard_normal((UTT, D_IN), dtype=np.float32)))
    post = [[(int(p), w) for p, w in zip(sorted(rng.choice(D_OUT, NNZ, replace=False)), (0.5, 0.375, 0.125))] for _ in range(UTT)]
    with open(os.path.join(tmp, "post.ark"), "wb") as f:
        f.write(b"u " + kf.posterior_bin(post))
    open(os.path.join(tmp, "nnet.proto"), "w").write(proto())


def write_scripts(tmp, tag, n_utt):
    for name in ("feats", "post"):
        with open(os.path.join(tmp, "%s_%s.scp" % (name, tag)), "w") as f:
            for i in range(n_utt):
                f.write("utt%05d %s:2\n" % (i, os.path.join(tmp, name + ".ark")))   # (2: behind the key "u " of the archive's one entry)


def tool_elapsed(tree, env, tmp, tag, mb, n_utt):
    exe = os.path.join(tree, "kaldi-aslp_amd", "bin", "aslp-nnet-train-frame")
    p = subprocess.run([exe, "--print-args=false", "--learn-rate=0.000001", "--minibatch-size=%d" % mb, "--randomizer-size=32768",
                        "scp:%s/feats_%s.scp" % (tmp, tag), "scp:%s/post_%s.scp" % (tmp, tag), tmp + "/nnet.init", tmp + "/nnet.out"],
                       env=env, capture_output=True, timeout=900)
    err = p.stderr.decode()
    m = re.search(r"min, fps([0-9.eE+-]+)\]", err)
    if p.returncode != 0 or not m:
        raise SystemExit("aslp-nnet-train-frame failed in %s:\n%s" % (tree, err[-2000:]))
    return n_utt * UTT / float(m.group(1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warm", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--forms", default="tool,step")
    ap.add_argument("builds", nargs="+")
    a = ap.parse_args()
    builds = []
    for b in a.builds:
        name, rest = b.split("=", 1)
        parts = rest.split(",")
        builds.append((name, os.path.abspath(parts[0]), dict(kv.split("=", 1) for kv in parts[1:])))
    tmp = a.tmp or tempfile.mkdtemp(prefix="xent_soft_step_")
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
                if "tool" in a.forms:
                    n_w, n_f = utts[mb]
                    t_w = tool_elapsed(tree, env, tmp, "warm%d" % mb, mb, n_w)
                    t_f = tool_elapsed(tree, env, tmp, "full%d" % mb, mb, n_f)
                    ms = (t_f - t_w) / ((n_f - n_w) * (UTT // mb)) * 1e3
                    samples.setdefault((name, "tool", mb), []).append(ms)
                    print("round %d %-8s tool  mb %4d: %.4f ms/step" % (rnd, name, mb, ms), flush=True)
                if "step" in a.forms:
                    p = subprocess.run([sys.executable, "-c", STEP_CHILD, tree, str(mb), str(a.warm), str(a.steps), tmp + "/nnet.proto"], env=env,
                                       capture_output=True, timeout=900)
                    m = re.search(r"STEP (\S+) (\S+)", p.stdout.decode())
                    if p.returncode != 0 or not m:
                        raise SystemExit("step child failed in %s:\n%s" % (tree, p.stderr.decode()[-2000:]))
                    samples.setdefault((name, "step", mb), []).append(float(m.group(2)))
                    print("round %d %-8s %-5s mb %4d: %.4f ms/step" % (rnd, name, m.group(1), mb, float(m.group(2))), flush=True)
    first = builds[0][0]
    print("\n%-8s %-5s %5s %10s %10s %12s  %s" % ("build", "form", "mb", "median ms", "spread ms", "vs " + first, "inside its spread"))
    for (name, form, mb), v in sorted(samples.items(), key=lambda kv: (kv[0][1], kv[0][2], [b[0] for b in builds].index(kv[0][0]))):
        med, spread = statistics.median(v), max(v) - min(v)
        rmed, rspread = statistics.median(samples[(first, form, mb)]), max(samples[(first, form, mb)]) - min(samples[(first, form, mb)])
        print("%-8s %-5s %5d %10.4f %10.4f %+11.2f%%  %s" % (name, form, mb, med, spread, (med / rmed - 1) * 100, "yes" if med <= rmed + rspread else "NO"))


if __name__ == "__main__":
    main()
