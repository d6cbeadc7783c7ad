"""The CTC losses on the device token-error path (nnet/ctc-token-errors.h: counted behind the loss, booked later) against the host loop
they replace: the same statistics as numbers, the same Report() as strings, the same tool logs line for line and the same models byte
for byte -- and the path a call took is the path it reports."""
import os
import subprocess

import numpy as np
import pytest
import torch

import ctc_errors_ref as ref
import kaldi_formats as kf
from test_ref_mains_diff_gpu import log_lines

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kaldi-aslp_amd", "bin")


@pytest.fixture(autouse=True)
def switch_back(aslp):
    yield
    aslp.ops.ctc_errors_on_host(-1)


def batches(seed, A=11, mb=5, maxT=36, n=3):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        in_len = rng.integers(maxT // 2, maxT + 1, mb).astype(np.int32)
        in_len[int(rng.integers(0, mb))] = maxT
        labels = [[int(v) for v in rng.integers(1, A, max(1, int(t) // 4))] for t in in_len]
        acts = np.repeat((rng.standard_normal((maxT // 2, mb, A)) * 2).astype(np.float32), 2, axis=0).reshape(maxT * mb, A)
        out.append((in_len, labels, acts))
    return out


def run_loss(aslp, dev, kind, on_host, data):
    """three batches through Eval + ErrorRate; returns what the book says after each batch and at the end, and the paths taken"""
    aslp.ops.ctc_errors_on_host(on_host)
    ctc = aslp.WarpCtc() if kind == "warp" else aslp.Ctc()
    seen, paths = [], []
    for in_len, labels, acts in data:
        x = torch.from_numpy(acts).to(dev)
        if kind == "warp":
            ctc.Eval(in_len, x, labels)
            ctc.ErrorRate(in_len, x, labels)
        else:
            y = torch.softmax(x, dim=1)
            ctc.EvalParallel(in_len, y, labels)
            ctc.ErrorRateMSeq(in_len, y, labels)
        paths.append(aslp.lib.aslp_ctc_errors_last_path())
        seen.append(ctc.GetStats())   # at once: the deferred form must have settled, not read early
    return seen, ctc.GetStats(), ctc.Report(), paths


@pytest.mark.parametrize("kind", ["warp", "eesen"])
def test_device_path_books_what_the_host_path_books(aslp, dev, kind):
    data = batches(5 if kind == "warp" else 6)
    seen_d, stats_d, report_d, paths_d = run_loss(aslp, dev, kind, 0, data)
    seen_h, stats_h, report_h, paths_h = run_loss(aslp, dev, kind, 1, data)
    assert paths_d == [1, 1, 1] and paths_h == [0, 0, 0]
    assert seen_d == seen_h and stats_d == stats_h
    assert report_d == report_h
    # ... and both book what the model counts, batch by batch
    err = refs = 0
    for (in_len, labels, acts), st in zip(data, seen_d):
        errors, _ = ref.token_errors(acts, labels, in_len)
        err += int(errors.sum())
        refs += sum(len(l) for l in labels)
        assert st["error_tokens"] == err and st["ref_tokens"] == refs


def test_single_sequence_error_rate(aslp, dev):
    rng = np.random.default_rng(9)
    acts = np.repeat(rng.standard_normal((20, 9)).astype(np.float32), 2, axis=0)
    label = [int(v) for v in rng.integers(1, 9, 11)]
    want, _ = ref.token_errors(acts, [label])
    y = torch.softmax(torch.from_numpy(acts).to(dev), dim=1)
    got = {}
    for on_host in (0, 1):
        aslp.ops.ctc_errors_on_host(on_host)
        ctc = aslp.Ctc()
        ctc.ErrorRate(y, label)
        assert aslp.lib.aslp_ctc_errors_last_path() == 1 - on_host
        got[on_host] = (ctc.GetStats(), ctc.Report())
        assert got[on_host][0]["error_tokens"] == int(want[0]) and got[on_host][0]["ref_tokens"] == len(label)
    assert got[0] == got[1]


def test_a_batch_the_kernel_does_not_serve_takes_the_host_path(aslp, dev):
    aslp.ops.ctc_errors_on_host(0)
    R = 1025   # one reference token more than the kernel serves (aslp_ctc_token_errors_supported)
    assert aslp.lib.aslp_ctc_token_errors_supported(60, R) == 0
    rng = np.random.default_rng(2)
    labels = [[int(v) for v in rng.integers(1, 6, R)], [1, 2, 3]]
    acts = rng.standard_normal((60 * 2, 6)).astype(np.float32)
    ctc = aslp.WarpCtc()
    ctc.ErrorRate([60, 41], torch.from_numpy(acts).to(dev), labels)
    assert aslp.lib.aslp_ctc_errors_last_path() == 0
    errors, _ = ref.token_errors(acts, labels, [60, 41])
    st = ctc.GetStats()
    assert st["error_tokens"] == int(errors.sum()) and st["ref_tokens"] == R + 3


# ---- end to end: the two stream tools with and without ASLP_CTC_ERRORS_HOST=1 ----------------------------------------------------------
CTC_PROTO = """<NnetProto>
<BLstmProjectedStreams> <InputDim> 12 <OutputDim> 16 <CellDim> 12 <ParamScale> 0.1 <ClipGradient> 5.0
<AffineTransform> <InputDim> 16 <OutputDim> 9 <BiasMean> 0.0 <BiasRange> 0.0 <ParamStddev> 0.1
%s</NnetProto>
"""


def run_tool(name, args, env_host):
    env = dict(os.environ)
    env.pop("ASLP_CTC_ERRORS_HOST", None)
    if env_host:
        env["ASLP_CTC_ERRORS_HOST"] = "1"
    p = subprocess.run([os.path.join(BIN, name)] + list(args), capture_output=True, timeout=1800, env=env)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    return p


@pytest.mark.parametrize("tool_name", ["aslp-nnet-train-warp-ctc-streams", "aslp-nnet-train-ctc-streams"])
def test_stream_tools_identical_under_the_switch(aslp, dev, tmp_path, tool_name):
    eesen = tool_name.endswith("-ctc-streams") and "warp" not in tool_name
    (tmp_path / "ctc.proto").write_text(CTC_PROTO % ("<Softmax> <InputDim> 9 <OutputDim> 9\n" if eesen else ""))
    run_tool("aslp-nnet-init", ["--seed=41", str(tmp_path / "ctc.proto"), str(tmp_path / "ctc.init")], False)
    rng = np.random.default_rng(21)
    n_utt, D, A = 12, 12, 9
    keys = ["u%02d" % i for i in range(n_utt)]
    lens = [int(x) for x in rng.integers(12, 40, n_utt)]
    feats = [rng.standard_normal((n, D)).astype(np.float32) for n in lens]
    labels = [[int(x) for x in rng.integers(1, A, max(1, n // 5))] for n in lens]
    (tmp_path / "feats.ark").write_bytes(kf.archive([(k, kf.matrix_bin(f)) for k, f in zip(keys, feats)]))
    (tmp_path / "lab.ark").write_bytes(kf.archive([(k, kf.int32vec_bin(l)) for k, l in zip(keys, labels)]))
    logs, models = [], []
    for env_host in (False, True):
        out = tmp_path / ("out%d.nnet" % env_host)
        # progress lines every 4 sequences and reports every 6, so both fall between batches of 3
        p = run_tool(tool_name, ["--learn-rate=0.5", "--momentum=0.9", "--num-stream=3", "--report-step=4", "--report-period=6",
                                 "ark:%s" % (tmp_path / "feats.ark"), "ark:%s" % (tmp_path / "lab.ark"), str(tmp_path / "ctc.init"), str(out)], env_host)
        logs.append([ln.replace(out.name, "out.nnet") for ln in log_lines(p.stderr)])
        models.append(out.read_bytes())
    assert models[0] == models[1]
    assert logs[0] == logs[1]
    text = "\n".join(logs[0])
    assert "TokenAcc" in text and text.count("TOKEN_ACCURACY") >= 3
