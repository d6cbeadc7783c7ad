"""End-to-end valid frames/s of the chunked stream tool on BASELINE cfg3: aslp-nnet-init -> aslp-nnet-train-blstm-streams-lc reading a
feature archive and a posterior archive from disk (page cache) behind a splice + shift/scale --feature-transform, 32 streams, chunk 40 +
right context 20.  devtools/bench_lc.py is the compute-only step of the same net (batch already on the device); this is the tool around it:
table reads, the transform per utterance, batch assembly, loss, model write.

  python devtools/bench_stream_tool_e2e.py [--tmp DIR] [--frames N] [--repeats R] [--warmup-rounds W] [--compute-fps F] [--leg NAME=BINDIR[,host]] ...

Each --leg names a build's bin/ directory (default: this tree's, once as `device` and once as `host` = ASLP_STREAM_BATCH_HOST=1); the legs
run in turn, R rounds (A B C A B C ...), and the median and the spread (max - min) of the tool's own fps line are printed per leg, with
the ratio to --compute-fps (the `valid frames/s` of bench_lc.py 32) when given."""
import argparse
import hashlib
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kaldi_formats as kf  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tmp", default="/tmp/stream_e2e")
ap.add_argument("--frames", type=int, default=600000)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--warmup-rounds", type=int, default=1)
ap.add_argument("--streams", type=int, default=32)
ap.add_argument("--compute-fps", type=float, default=0.0)
ap.add_argument("--leg", action="append", default=[])
args = ap.parse_args()
own = os.path.join(ROOT, "kaldi-aslp_amd", "bin")
legs = []
for spec in args.leg or ["device=" + own, "host=" + own + ",host"]:
    name, rest = spec.split("=", 1)
    parts = rest.split(",")
    legs.append((name, parts[0], "host" in parts[1:]))

tmp = args.tmp
os.makedirs(tmp, exist_ok=True)
RAW, CTX, CHUNK, RIGHT, A = 8, 2, 40, 20, 3000
D = RAW * (2 * CTX + 1)   # 40: cfg3's input
proto = ["<NnetProto>"]
d = D
for _ in range(4):
    proto.append("<BLstmProjectedStreamsLC> <InputDim> %d <OutputDim> 512 <CellDim> 512 <ParamScale> 0.02 <ClipGradient> 5.0" % d)
    d = 512
proto += ["<AffineTransform> <InputDim> 512 <OutputDim> %d <BiasMean> 0.0 <BiasRange> 0.0 <ParamStddev> 0.04" % A,
          "<Softmax> <InputDim> %d <OutputDim> %d" % (A, A), "</NnetProto>"]
open(tmp + "/nnet.proto", "w").write("\n".join(proto) + "\n")
open(tmp + "/tr.proto", "w").write("<NnetProto>\n<Splice> <InputDim> %d <OutputDim> %d <BuildVector> -%d:%d </BuildVector>\n"
                                   "<AddShift> <InputDim> %d <OutputDim> %d <InitParam> 0.1\n<Rescale> <InputDim> %d <OutputDim> %d <InitParam> 0.5\n</NnetProto>\n"
                                   % (RAW, D, CTX, CTX, D, D, D, D))
rng = np.random.default_rng(0)
total = 0
with open(tmp + "/feats.ark", "wb") as ff, open(tmp + "/post.ark", "wb") as pf:
    i = 0
    while total < args.frames:
        T = int(rng.integers(200, 601))   # utterances of a few hundred frames: some stream takes a new one in almost every step
        ff.write(("utt%05d " % i).encode() + kf.matrix_bin(rng.standard_normal((T, RAW), dtype=np.float32)))
        pf.write(("utt%05d " % i).encode() + kf.posterior_bin([[(int(l), 1.0)] for l in rng.integers(0, A, T)]))
        total += T
        i += 1
print("corpus: %d utterances, %d frames" % (i, total))
subprocess.run([own + "/aslp-nnet-init", "--print-args=false", "--seed=777", tmp + "/nnet.proto", tmp + "/nnet.init"], check=True, capture_output=True)
subprocess.run([own + "/aslp-nnet-init", "--print-args=false", tmp + "/tr.proto", tmp + "/tr.nnet"], check=True, capture_output=True)

fps = {name: [] for name, _, _ in legs}
walls = {name: [] for name, _, _ in legs}
models = set()
for rnd in range(-args.warmup_rounds, args.repeats):   # rounds < 0 warm the page cache and the code objects and are not counted
    for name, bindir, host in legs:
        env = dict(os.environ)
        env.pop("ASLP_STREAM_BATCH_HOST", None)
        if host:
            env["ASLP_STREAM_BATCH_HOST"] = "1"
        t0 = time.time()
        p = subprocess.run([bindir + "/aslp-nnet-train-blstm-streams-lc", "--print-args=false", "--learn-rate=0.00001", "--momentum=0.9",
                            "--num-stream=%d" % args.streams, "--chunk-size=%d" % CHUNK, "--right-splice=%d" % RIGHT, "--report-period=100000",
                            "--feature-transform=%s/tr.nnet" % tmp, "ark:%s/feats.ark" % tmp, "ark:%s/post.ark" % tmp, tmp + "/nnet.init",
                            tmp + "/nnet.out"], capture_output=True, env=env, timeout=900)
        wall = time.time() - t0
        err = p.stderr.decode()
        if p.returncode != 0:
            print(err[-2000:])
            sys.exit("leg %s failed with exit status %d" % (name, p.returncode))
        m = re.search(r"min, fps([-+0-9.e]+)\]", err)
        if rnd >= 0:
            fps[name].append(float(m.group(1)))
            walls[name].append(wall)
        models.add(hashlib.sha1(open(tmp + "/nnet.out", "rb").read()).hexdigest())
        loss = [ln for ln in err.splitlines() if "AvgLoss" in ln][-1:]
        print("round %d  %-8s tool fps %.0f  process wall %.2f s  %s" % (rnd, name, float(m.group(1)), wall, loss[0].split(")")[-1].strip() if loss else ""))
for name, _, _ in legs:
    v = fps[name]
    line = "%-8s valid frames/s: median %.0f  spread %.0f (min %.0f max %.0f, n=%d); process wall median %.2f s" % (
        name, statistics.median(v), max(v) - min(v), min(v), max(v), len(v), statistics.median(walls[name]))
    if args.compute_fps > 0:
        line += "; %.3f of the compute-only step (%.0f)" % (statistics.median(v) / args.compute_fps, args.compute_fps)
    print(line)
print("models written by all runs of all legs: %s" % ("byte-identical" if len(models) == 1 else "%d DIFFERENT files" % len(models)))
