"""The chunked stream tools with their batches gathered on the device (the default) and assembled on the host (ASLP_STREAM_BATCH_HOST=1):
aslp-nnet-train-blstm-streams-lc and aslp-nnet-train-lstm-streams-skip behind a --feature-transform, 7 utterances on 3 streams.  The switch
moves where a batch is put together and nothing else: the models must be byte-identical and the logs equal once times are masked."""
import os
import subprocess

import numpy as np
import pytest

import kaldi_formats as kf
from test_ref_mains_diff_gpu import log_lines

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kaldi-aslp_amd", "bin")

RAW, CTX, A = 4, 1, 10
NET_IN = RAW * (2 * CTX + 1)
TRANSFORM = """<NnetProto>
<Splice> <InputDim> %d <OutputDim> %d <BuildVector> -%d:%d </BuildVector>
<AddShift> <InputDim> %d <OutputDim> %d <InitParam> 0.25
<Rescale> <InputDim> %d <OutputDim> %d <InitParam> 0.5
</NnetProto>
""" % (RAW, NET_IN, CTX, CTX, NET_IN, NET_IN, NET_IN, NET_IN)
PROTOS = {
    "aslp-nnet-train-blstm-streams-lc": "<BLstmProjectedStreamsLC> <InputDim> %d <OutputDim> 16 <CellDim> 12 <ParamScale> 0.1 <ClipGradient> 5.0" % NET_IN,
    "aslp-nnet-train-lstm-streams-skip": "<LstmProjectedStreams> <InputDim> %d <OutputDim> 16 <CellDim> 12 <ParamScale> 0.1 <ClipGradient> 5.0" % NET_IN,
}
FLAGS = {
    "aslp-nnet-train-blstm-streams-lc": ["--chunk-size=6", "--right-splice=3"],
    "aslp-nnet-train-lstm-streams-skip": ["--batch-size=5", "--targets-delay=2", "--skip-width=2"],
}


def run_tool(name, args, on_host):
    env = dict(os.environ)
    env.pop("ASLP_STREAM_BATCH_HOST", None)
    if on_host:
        env["ASLP_STREAM_BATCH_HOST"] = "1"
    p = subprocess.run([os.path.join(BIN, name)] + list(args), capture_output=True, timeout=1800, env=env)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    return p


@pytest.mark.parametrize("tool_name", sorted(PROTOS))
def test_stream_tools_identical_under_the_switch(dev, tmp_path, tool_name):
    (tmp_path / "net.proto").write_text("<NnetProto>\n%s\n<AffineTransform> <InputDim> 16 <OutputDim> %d <BiasMean> 0.0 <BiasRange> 0.0 <ParamStddev> 0.1\n"
                                        "<Softmax> <InputDim> %d <OutputDim> %d\n</NnetProto>\n" % (PROTOS[tool_name], A, A, A))
    (tmp_path / "tr.proto").write_text(TRANSFORM)
    run_tool("aslp-nnet-init", ["--seed=61", str(tmp_path / "net.proto"), str(tmp_path / "net.init")], False)
    run_tool("aslp-nnet-init", ["--seed=62", str(tmp_path / "tr.proto"), str(tmp_path / "tr.nnet")], False)
    rng = np.random.default_rng(31)
    lens = [1, 9, 23, 4, 15, 30, 12]   # 7 utterances; 9 = one batch of the LC tool, 1 = shorter than delay and skip
    keys = ["v%02d" % i for i in range(len(lens))]
    feats = [rng.standard_normal((n, RAW)).astype(np.float32) for n in lens]
    posts = [[[(int(rng.integers(0, A)), 1.0)] for _ in range(n)] for n in lens]
    (tmp_path / "feats.ark").write_bytes(kf.archive([(k, kf.matrix_bin(f)) for k, f in zip(keys, feats)]))
    (tmp_path / "post.ark").write_bytes(kf.archive([(k, kf.posterior_bin(p)) for k, p in zip(keys, posts)]))
    logs, models = [], []
    for on_host in (False, True):
        out = tmp_path / ("out%d.nnet" % on_host)
        p = run_tool(tool_name, ["--learn-rate=0.05", "--momentum=0.9", "--num-stream=3", "--report-period=2", "--feature-transform=%s" % (tmp_path / "tr.nnet")]
                     + FLAGS[tool_name] + ["ark:%s" % (tmp_path / "feats.ark"), "ark:%s" % (tmp_path / "post.ark"), str(tmp_path / "net.init"), str(out)], on_host)
        logs.append([ln.replace(out.name, "out.nnet") for ln in log_lines(p.stderr)])
        models.append(out.read_bytes())
    assert models[0] == models[1]
    assert logs[0] == logs[1]
    text = "\n".join(logs[0])
    assert "AvgLoss" in text and "Done " in text
