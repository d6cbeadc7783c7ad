"""Tanh and ReLU hidden layers on the engine's fast layer path: the activation (and the planes / maxima its consumer needs) from the
product's epilogue, the backward kernels that write planes, the A/B switch ASLP_FUSE_TANH_RELU.  Environment switches are read once per
process, so every setting trains the same three small nets in a child process (as tests/test_dnn_ab_switches_gpu.py does) for two steps
with momentum 0.9 and hands back outputs, first-layer in-diffs, parameters and Nnet.LastFusedActivations(); the parent compares the
settings with each other and with the oracle chain (orc_relu, orc_tanh, orc_diff_*).

  chain:  AffineTransform 100->256, ReLU, AffineTransform 256->320, Tanh, AffineTransform 320->132, ReLU, AffineTransform 132->40, Softmax
  fork:   a graph net whose ReLU feeds two AffineTransforms (not fused)
  linear: AffineTransform 160->256, ReLU, AffineTransform 256->192, ReLU, LinearTransform 192->128, Softmax (the second ReLU's consumer is
          no AffineTransform: fused, no planes; the first ReLU's backward pass writes the lower layer's out-diff planes)
Minibatch 192 (one and a half tile rows)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nnet_io
from test_dnn_ab_switches_gpu import ROOT, close

pytestmark = pytest.mark.gpu
MB, LR, MMT, STEPS, TOL = 192, 0.01, 0.9, 2, 1e-4

CHILD = r'''
import sys, os
import numpy as np, torch
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import aslp_import
aslp = aslp_import.load(); aslp.ops.use_torch_stream()
dev = torch.device("cuda:0")
work, out_path = sys.argv[1], sys.argv[2]
data = np.load(os.path.join(work, "data.npz"))
res = {}
for name in ("chain", "fork", "linear"):
    for fusion in (1, 0):
        net = aslp.Nnet.Read(os.path.join(work, name + ".nnet"))
        net.SetLayerFusion(fusion)
        net.SetTrainOptions(learn_rate=%(lr)r, momentum=%(mmt)r)
        key = "%%s.%%d." %% (name, fusion)
        for step in range(%(steps)d):
            out = net.Propagate(torch.from_numpy(data[name + ".x"][step]).to(dev))
            res[key + "fused%%d" %% step] = np.int64(net.LastFusedActivations())
            idf = net.Backpropagate(torch.from_numpy(data[name + ".od"][step]).to(dev), want_in_diff=True)
            res[key + "out%%d" %% step] = out.cpu().numpy()
            res[key + "idf%%d" %% step] = idf.cpu().numpy()
            res[key + "par%%d" %% step] = np.asarray(net.GetParams(), np.float32)
np.savez(out_path, **res)
'''

SETTINGS = {"default": {}, "switch_off": {"ASLP_FUSE_TANH_RELU": "0"}, "fp32": {"ASLP_GEMM_SPLIT_F16": "0"},
            "fp32_switch_off": {"ASLP_GEMM_SPLIT_F16": "0", "ASLP_FUSE_TANH_RELU": "0"}}


def _affine(rng, din, dout):
    return (rng.standard_normal((dout, din)) * (1.0 / np.sqrt(din))).astype(np.float32), (rng.standard_normal(dout) * 0.5).astype(np.float32)


def _linear_data(W):
    return nnet_io.tok("<LearnRateCoef>") + nnet_io.f32(1.0) + nnet_io.fmat(W)


@pytest.fixture(scope="module")
def nets():
    """the three nets' weights, in layer order: ("affine", W, b) | ("linear", W) | ("relu",) | ("tanh",) | ("softmax",)"""
    rng = np.random.default_rng(17)
    chain = [("affine",) + _affine(rng, 100, 256), ("relu",), ("affine",) + _affine(rng, 256, 320), ("tanh",),
             ("affine",) + _affine(rng, 320, 132), ("relu",), ("affine",) + _affine(rng, 132, 40), ("softmax",)]
    linear = [("affine",) + _affine(rng, 160, 256), ("relu",), ("affine",) + _affine(rng, 256, 192), ("relu",),
              ("linear", (rng.standard_normal((128, 192)) / np.sqrt(192.0)).astype(np.float32)), ("softmax",)]
    fork = [_affine(rng, 100, 256), _affine(rng, 256, 128), _affine(rng, 256, 128), _affine(rng, 256, 40)]   # a1 -> relu -> (a2a, a2b) -> a3
    return dict(chain=chain, linear=linear, fork=fork)


def _simple_layers(layers):
    out, d = [], None
    for l in layers:
        if l[0] == "affine":
            out.append(("<AffineTransform>", l[1].shape[1], l[1].shape[0], nnet_io.affine(l[1], l[2])))
            d = l[1].shape[0]
        elif l[0] == "linear":
            out.append(("<LinearTransform>", l[1].shape[1], l[1].shape[0], _linear_data(l[1])))
            d = l[1].shape[0]
        else:
            out.append(({"relu": "<ReLU>", "tanh": "<Tanh>", "softmax": "<Softmax>"}[l[0]], d, d, b""))
    return out


@pytest.fixture(scope="module")
def runs(nets, tmp_path_factory):
    """every setting's child process, started together (four processes on the device), and the inputs they all read"""
    work = tmp_path_factory.mktemp("act_fusion")
    rng = np.random.default_rng(23)
    nnet_io.write_simple_nnet(work / "chain.nnet", _simple_layers(nets["chain"]))
    nnet_io.write_simple_nnet(work / "linear.nnet", _simple_layers(nets["linear"]))
    (W1, b1), (Wa, ba), (Wb, bb), (W3, b3) = nets["fork"]
    nnet_io.write_graph_nnet(work / "fork.nnet", [
        dict(marker="<InputLayer>", dim_in=100, dim_out=100, id=0, inputs=[-1], offsets=[0]),
        dict(marker="<AffineTransform>", dim_in=100, dim_out=256, id=1, inputs=[0], offsets=[0], data=nnet_io.affine(W1, b1)),
        dict(marker="<ReLU>", dim_in=256, dim_out=256, id=2, inputs=[1], offsets=[0]),
        dict(marker="<AffineTransform>", dim_in=256, dim_out=128, id=3, inputs=[2], offsets=[0], data=nnet_io.affine(Wa, ba)),
        dict(marker="<AffineTransform>", dim_in=256, dim_out=128, id=4, inputs=[2], offsets=[0], data=nnet_io.affine(Wb, bb)),
        dict(marker="<AffineTransform>", dim_in=256, dim_out=40, id=5, inputs=[3, 4], offsets=[0, 128], data=nnet_io.affine(W3, b3)),
        dict(marker="<OutputLayer>", dim_in=40, dim_out=40, id=6, inputs=[5], offsets=[0]),
    ])
    data = {}
    for name, din, dout in (("chain", 100, 40), ("fork", 100, 40), ("linear", 160, 128)):
        data[name + ".x"] = rng.standard_normal((STEPS, MB, din)).astype(np.float32)
        data[name + ".od"] = (rng.standard_normal((STEPS, MB, dout)) * 0.05).astype(np.float32)
    np.savez(work / "data.npz", **data)
    procs = {}
    for name, env in SETTINGS.items():
        procs[name] = subprocess.Popen([sys.executable, "-c", CHILD % dict(root=ROOT, lr=LR, mmt=MMT, steps=STEPS), str(work), str(work / (name + ".npz"))],
                                       env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    res = {}
    for name, p in procs.items():
        _, err = p.communicate(timeout=300)
        assert p.returncode == 0, (name, err.decode()[-2000:])
        res[name] = dict(np.load(work / (name + ".npz")))
    return res, data


def test_fused_activation_counts(runs):
    """the test that fails without the feature: the count does not exist there.  Three Tanh / ReLU layers ride in their products in the
    chain; the ReLU with two consumers does not; both ReLUs of the LinearTransform net do; none under SetLayerFusion(False) or the switch."""
    res, _ = runs
    for step in range(STEPS):
        for setting in ("default", "fp32"):
            r = res[setting]
            assert (r["chain.1.fused%d" % step], r["fork.1.fused%d" % step], r["linear.1.fused%d" % step]) == (3, 0, 2), (setting, step)
            assert (r["chain.0.fused%d" % step], r["fork.0.fused%d" % step], r["linear.0.fused%d" % step]) == (0, 0, 0), (setting, step)
        for setting in ("switch_off", "fp32_switch_off"):
            for key in ("chain.1", "chain.0", "fork.1", "linear.1"):
                assert res[setting]["%s.fused%d" % (key, step)] == 0, (setting, key, step)


def _tensors(r, key):
    return [(what + str(step), r["%s.%s%d" % (key, what, step)]) for step in range(STEPS) for what in ("out", "idf", "par")]


def test_fp32_instruction_fused_is_bit_identical(runs):
    """no planes anywhere: the only difference between the fused and the unfused run is the kernel in which act(v) is evaluated"""
    res, _ = runs
    for name in ("chain", "fork", "linear"):
        fused = _tensors(res["fp32"], name + ".1")
        for other, key in (("fp32", name + ".0"), ("fp32_switch_off", name + ".1")):
            for (what, a), (_, b) in zip(fused, _tensors(res[other], key)):
                assert np.array_equal(a, b), (name, other, key, what)


def test_default_path_fused_close_to_unfused(runs):
    """on the split-fp16 path the planes of a fused layer are scaled by another bound than a conversion finds (1 against max |tanh|, max |od|
    against max |in-diff|): values agree to fp32 rounding -- the bound tests/test_dnn_ab_switches_gpu.py puts on such switches (its close)"""
    res, _ = runs
    one = np.ones(1)
    for name in ("chain", "fork", "linear"):
        fused = _tensors(res["default"], name + ".1")
        for other, key in (("default", name + ".0"), ("switch_off", name + ".1"), ("fp32", name + ".1")):
            for (what, a), (_, b) in zip(fused, _tensors(res[other], key)):
                a, b = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
                print(name, other, key, what, "rel", np.linalg.norm(a - b) / np.linalg.norm(b))
                assert close(np.concatenate([one, a]), np.concatenate([one, b])), (name, other, key, what)


class _Chain:
    """the oracle's forward / backward / update over a simple net's layers"""

    def __init__(self, oracle, layers):
        self.o = oracle
        self.layers = [(l[0], oracle.Affine(l[1], l[2]) if l[0] == "affine" else oracle.Linear(l[1]) if l[0] == "linear" else None) for l in layers]

    def params(self):
        return np.concatenate([np.concatenate([c.W.ravel(), c.b]) if k == "affine" else c.W.ravel() for k, c in self.layers if c is not None])

    def grads(self):
        g = []
        for i, (k, c) in enumerate(self.layers):
            if k == "affine":
                g += [("W%d" % i, c.Wc), ("b%d" % i, c.bc)]
            elif k == "linear":
                g.append(("W%d" % i, c.corr))
        return g

    def step(self, x, od):
        o, ins, outs = self.o, [], []
        for k, c in self.layers:
            ins.append(x)
            x = c.propagate(x) if c is not None else o.unary({"relu": "orc_relu", "tanh": "orc_tanh", "softmax": "orc_softmax_rows"}[k], x)
            outs.append(x)
        d, diffs = od, [None] * len(self.layers)
        for i in reversed(range(len(self.layers))):
            k, c = self.layers[i]
            diffs[i] = d
            if c is not None:
                d = c.backpropagate(d)
            elif k == "relu":
                d = o.binary("orc_diff_relu", ins[i], d)
            elif k == "tanh":
                d = o.binary("orc_diff_tanh", outs[i], d)
            # (Softmax: the backward pass is a copy, nnet-activation.h:51-59)
        for i, (k, c) in enumerate(self.layers):
            if c is not None:
                c.update(ins[i], diffs[i], LR, MMT)
        return outs[-1], d


def _check_against_oracle(oracle, r, key, step_fn, params_fn, grads_fn, x, od, what):
    prev = params_fn()
    for step in range(STEPS):
        out_ref, idf_ref = step_fn(x[step], od[step])
        out, idf, par = r["%s.out%d" % (key, step)], r["%s.idf%d" % (key, step)], r["%s.par%d" % (key, step)]
        errs = (oracle.rel_err(out, out_ref), oracle.rel_err(idf, idf_ref), oracle.rel_err(par, params_fn()))
        print(what, key, "step", step, "rel err out / in-diff / params", errs)
        assert max(errs) < TOL, (what, key, step, errs)
        assert oracle.max_err(out, out_ref) < 10 * TOL and oracle.max_err(idf, idf_ref) < 10 * TOL, (what, key, step)
        before = prev if step == 0 else r["%s.par%d" % (key, step - 1)]
        oracle.assert_applied_gradients(before, par, LR, grads_fn(), tol=TOL, what="%s %s step %d" % (what, key, step))


@pytest.mark.parametrize("name", ["chain", "linear"])
def test_fused_runs_match_the_oracle(runs, nets, oracle, name):
    """outputs, first-layer in-diff, every updated parameter and the applied gradient of every tensor at the project's fp32 parity bound"""
    res, data = runs
    for setting in ("default", "fp32"):
        ch = _Chain(oracle, nets[name])
        _check_against_oracle(oracle, res[setting], name + ".1", ch.step, ch.params, ch.grads, data[name + ".x"], data[name + ".od"], setting)


def test_relu_with_two_consumers_matches_the_oracle(runs, nets, oracle):
    res, data = runs
    for setting in ("default", "fp32"):
        a1, a2a, a2b, a3 = (oracle.Affine(W, b) for W, b in nets["fork"])

        def step(x, od):
            p1 = a1.propagate(x)
            h = oracle.unary("orc_relu", p1)
            ya, yb = a2a.propagate(h), a2b.propagate(h)
            cat = np.concatenate([ya, yb], 1)
            out = a3.propagate(cat)
            dcat = a3.backpropagate(od)
            da, db = np.ascontiguousarray(dcat[:, :128]), np.ascontiguousarray(dcat[:, 128:])
            dh = a2a.backpropagate(da) + a2b.backpropagate(db)
            d1 = oracle.binary("orc_diff_relu", p1, dh)
            idf = a1.backpropagate(d1)
            for c, xin, d in ((a1, x, d1), (a2a, h, da), (a2b, h, db), (a3, cat, od)):
                c.update(xin, d, LR, MMT)
            return out, idf

        params = lambda: np.concatenate([np.concatenate([c.W.ravel(), c.b]) for c in (a1, a2a, a2b, a3)])
        grads = lambda: [g for i, c in enumerate((a1, a2a, a2b, a3)) for g in (("W%d" % i, c.Wc), ("b%d" % i, c.bc))]
        _check_against_oracle(oracle, res[setting], "fork.1", step, params, grads, data["fork.x"], data["fork.od"], setting)
