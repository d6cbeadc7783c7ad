"""Xent on soft targets through the engine: Xent.EvalSparse and Nnet.train_step_xent_sparse (the C ABI under them) against the dense
routes they replace, and the command-line tools under the A/B switch ASLP_XENT_SPARSE.

The dense routes are the yardstick: Xent.Eval(targets=<csr -> dense>) for the loss class, Propagate + Xent.Eval(targets=dense) +
Backpropagate for the training step, and ASLP_XENT_SPARSE=0 (PosteriorToMatrix and the dense kernel, as before) for the tools.  A target
of 0 adds exactly 0 to every sum, and the row statistics the sparse route defers are summed with the bits of one sum per batch, so
everything is compared bit for bit."""
import os
import subprocess

import numpy as np
import pytest
import torch

import kaldi_formats as kf
import xent_sparse_ref as sp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "kaldi-aslp_amd", "bin")


def soft_posterior(rng, rows, cols, one_hot_every=0):
    """1 - 3 (pdf, weight) pairs per frame, the weights multiples of 1/8 that sum to 1; every one_hot_every-th frame one-hot"""
    post = []
    for r in range(rows):
        n = 1 if one_hot_every and r % one_hot_every == 0 else int(rng.integers(1, 4))
        pdfs = rng.choice(cols, n, replace=False)
        w = {1: [1.0], 2: [0.625, 0.375], 3: [0.5, 0.375, 0.125]}[n]
        post.append([(int(p), float(x)) for p, x in zip(pdfs, w)])
    return post


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("rows,cols", [(16, 1024), (8, 3000)])
def test_eval_sparse_is_eval_on_the_dense_matrix(aslp, dev, rows, cols):
    rng = np.random.default_rng(rows + cols)
    sparse, dense = aslp.Xent(), aslp.Xent()
    for b in range(3):
        post = soft_posterior(rng, rows, cols)
        post[b] = []                                                   # a frame without targets
        post[3 + b] = post[3 + b] + [(post[3 + b][0][0], 0.25)]        # a duplicate: the later one wins
        y = torch.softmax(torch.from_numpy(rng.standard_normal((rows, cols)).astype(np.float32) * 3).to(dev), 1)
        fw = torch.from_numpy(rng.choice(np.array([0.0, 0.5, 1.0, 1.0], np.float32), rows)).to(dev)
        rb, c, w = aslp.nnet.posterior_to_csr(post, cols, dev)
        want = sp.posterior_to_csr(post, cols)
        assert all(np.array_equal(a.cpu().numpy(), b_) for a, b_ in zip((rb, c, w), want))
        tgt = torch.from_numpy(sp.posterior_to_matrix(post, cols)).to(dev)
        d_sparse, d_dense = torch.full_like(y, 7.0), torch.full_like(y, 9.0)
        sparse.EvalSparse(fw, y, d_sparse, rb, c, w)
        dense.Eval(fw, y, d_dense, targets=tgt)
        assert torch.equal(d_sparse.view(torch.int32), d_dense.view(torch.int32)), b
    a, b = sparse.GetStats(), dense.GetStats()
    assert a["frames"] > 0 and all(bits(np.float64(a[k])) == bits(np.float64(b[k])) for k in a), (a, b)
    assert sparse.Report() == dense.Report() and "FRAME_ACCURACY" in sparse.Report()


def test_eval_sparse_reads_nothing_back(aslp, dev):
    rows, cols = 16, 1024
    rng = np.random.default_rng(5)
    xent = aslp.Xent()
    y = torch.softmax(torch.from_numpy(rng.standard_normal((rows, cols)).astype(np.float32)).to(dev), 1)
    rb, c, w = aslp.nnet.posterior_to_csr(soft_posterior(rng, rows, cols), cols, dev)
    fw, diff = torch.ones(rows, device=dev), torch.empty_like(y)
    xent.EvalSparse(fw, y, diff, rb, c, w)
    before = aslp.ops.device_to_host_syncs()
    for _ in range(40):                                                # (more batches than the deferred statistics hold at once)
        xent.EvalSparse(fw, y, diff, rb, c, w)
    assert aslp.ops.device_to_host_syncs() == before
    assert xent.GetStats()["frames"] == 41 * rows


def proto(out):
    return ("<NnetProto>\n"
            "<AffineTransform> <InputDim> 20 <OutputDim> 64 <BiasMean> -0.5 <BiasRange> 1.0 <ParamStddev> 0.1\n"
            "<Sigmoid> <InputDim> 64 <OutputDim> 64\n"
            "<AffineTransform> <InputDim> 64 <OutputDim> %d <BiasMean> 0.0 <BiasRange> 0.0 <ParamStddev> 0.1\n"
            "<Softmax> <InputDim> %d <OutputDim> %d\n</NnetProto>\n" % (out, out, out))


def two_steps(aslp, dev, out, composed):
    rows = 32
    rng = np.random.default_rng(100 + out)
    net = aslp.Nnet.Init(proto(out), seed=21)
    net.SetTrainOptions(learn_rate=0.02, momentum=0.5)
    xent = aslp.Xent()
    params, folds = [], []
    for _ in range(2):
        x = torch.from_numpy(rng.standard_normal((rows, 20)).astype(np.float32)).to(dev)
        post = soft_posterior(rng, rows, out)
        fw = torch.from_numpy(rng.choice(np.array([0.0, 0.5, 1.0, 2.0], np.float32), rows)).to(dev)
        if composed:
            y = net.Propagate(x)
            diff = torch.empty_like(y)
            xent.Eval(fw, y, diff, targets=torch.from_numpy(sp.posterior_to_matrix(post, out)).to(dev))
            net.Backpropagate(diff)
        else:
            net.train_step_xent_sparse(xent, x, *aslp.nnet.posterior_to_csr(post, out, dev), frame_weights=fw)
            folds.append(net.LastLossFold())
        params.append(net.GetParams().copy())
    return np.stack(params), xent.GetStats(), xent.Report(), folds


@pytest.mark.parametrize("split16", [0, -1], ids=["fp32-products", "default-products"])
@pytest.mark.parametrize("out", [600, 40], ids=["fold", "no-fold"])
def test_train_step_matches_the_composed_step(aslp, dev, out, split16):
    """20 -> 64 Sigmoid -> out Softmax, 32 rows, two steps.  At 600 classes the final Softmax is left to the loss kernel, at 40 it is not.
    Neither route writes planes of the diff, so the default products see the same operands as well: bit-identical on both legs (measured
    on an MI355X)."""
    aslp.lib.aslp_gemm_split16(split16)
    try:
        p_step, st_step, rep_step, folds = two_steps(aslp, dev, out, False)
        p_comp, st_comp, rep_comp, _ = two_steps(aslp, dev, out, True)
    finally:
        aslp.lib.aslp_gemm_split16(-1)
    assert folds == [1 if out > 512 else 0] * 2
    assert np.isfinite(p_step).all() and not np.array_equal(p_step[0], p_step[1])
    same = [np.array_equal(bits(a), bits(b)) for a, b in zip(p_step, p_comp)]
    print("out %d split16 %d: steps bit-identical %s" % (out, split16, same))
    assert all(same)
    assert all(bits(np.float64(st_step[k])) == bits(np.float64(st_comp[k])) for k in st_step), (st_step, st_comp)
    assert rep_step == rep_comp


def test_train_step_without_frame_weights_is_ones(aslp, dev):
    rows, out = 32, 40
    rng = np.random.default_rng(8)
    x = torch.from_numpy(rng.standard_normal((rows, 20)).astype(np.float32)).to(dev)
    csr = aslp.nnet.posterior_to_csr(soft_posterior(rng, rows, out), out, dev)
    got = []
    for fw in (None, torch.ones(rows, device=dev)):
        net = aslp.Nnet.Init(proto(out), seed=22)
        net.SetTrainOptions(learn_rate=0.02, momentum=0.0)
        net.train_step_xent_sparse(aslp.Xent(), x, *csr, frame_weights=fw)
        got.append(net.GetParams())
    assert np.array_equal(bits(got[0]), bits(got[1]))


# ---- the tools under the switch ----------------------------------------------------------------------------------------------------------
def log_lines(stderr):
    return [ln for ln in stderr.decode().splitlines() if "AvgLoss" in ln or "FRAME_ACCURACY" in ln]


def run_tool(name, args, sparse):
    env = dict(os.environ)
    env.pop("ASLP_XENT_SPARSE", None)
    if not sparse:
        env["ASLP_XENT_SPARSE"] = "0"
    exe = os.path.join(BIN, name)
    assert os.path.exists(exe), "%s not built (make -C kaldi-aslp_amd)" % exe
    p = subprocess.run([exe] + list(args), capture_output=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    return p


TOOLS = {
    # the frame tool at 520 classes: the final Softmax is left to the loss; the stream tool at 10: it is not
    "aslp-nnet-train-frame": (520, "<AffineTransform> <InputDim> 6 <OutputDim> 16 <BiasMean> -0.5 <BiasRange> 1.0 <ParamStddev> 0.1\n"
                                   "<Sigmoid> <InputDim> 16 <OutputDim> 16",
                              ["--minibatch-size=16", "--randomizer-size=64", "--randomizer-seed=3"]),
    "aslp-nnet-train-lstm-streams": (10, "<LstmProjectedStreams> <InputDim> 6 <OutputDim> 16 <CellDim> 12 <ParamScale> 0.1 <ClipGradient> 5.0",
                                     ["--num-stream=3", "--batch-size=5", "--targets-delay=2", "--report-period=2"]),
}


@pytest.mark.parametrize("tool_name", sorted(TOOLS))
def test_tools_identical_under_the_switch(dev, tmp_path, tool_name):
    A, body, flags = TOOLS[tool_name]
    (tmp_path / "net.proto").write_text("<NnetProto>\n%s\n<AffineTransform> <InputDim> 16 <OutputDim> %d <BiasMean> 0.0 <BiasRange> 0.0 <ParamStddev> 0.1\n"
                                        "<Softmax> <InputDim> %d <OutputDim> %d\n</NnetProto>\n" % (body, A, A, A))
    run_tool("aslp-nnet-init", ["--seed=61", str(tmp_path / "net.proto"), str(tmp_path / "net.init")], True)
    rng = np.random.default_rng(41)
    lens = [9, 23, 4, 15, 30, 12]
    keys = ["v%02d" % i for i in range(len(lens))]
    feats = [rng.standard_normal((n, 6)).astype(np.float32) for n in lens]
    posts = [soft_posterior(rng, n, A, one_hot_every=3) for n in lens]      # one-hot frames and frames of 2 - 3 pairs in one archive
    posts[1][1] = [(7, 0.25), (3, 0.5), (7, 0.5)]                             # a duplicate pdf within a frame: the later one wins
    assert any(len(f) == 1 for p in posts for f in p) and any(len(f) >= 2 for p in posts for f in p)
    (tmp_path / "feats.ark").write_bytes(kf.archive([(k, kf.matrix_bin(f)) for k, f in zip(keys, feats)]))
    (tmp_path / "post.ark").write_bytes(kf.archive([(k, kf.posterior_bin(p)) for k, p in zip(keys, posts)]))
    logs, models = [], []
    for sparse in (True, False):
        out = tmp_path / ("out%d.nnet" % sparse)
        p = run_tool(tool_name, ["--learn-rate=0.05", "--momentum=0.9"] + flags +
                     ["ark:%s" % (tmp_path / "feats.ark"), "ark:%s" % (tmp_path / "post.ark"), str(tmp_path / "net.init"), str(out)], sparse)
        logs.append([ln.replace(out.name, "out.nnet") for ln in log_lines(p.stderr)])
        models.append(out.read_bytes())
    assert models[0] == models[1] and models[0] != (tmp_path / "net.init").read_bytes()
    assert logs[0] == logs[1]
    text = "\n".join(logs[0])
    assert "AvgLoss" in text and "FRAME_ACCURACY" in text
