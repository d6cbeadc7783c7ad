"""One-plane layer products (aslp_gemm_operand_planes(1) / ASLP_GEMM_PLANES=1, csrc/gemm_split16.hip): the product kernels read the hi
plane of each operand alone -- operands X16 = fp16(X 2^up) 2^-up behind the per-matrix power-of-two scale, one matrix instruction per k
step, fp32 accumulation, the fp32 epilogue.  The contract checked here: against the product of the ROUNDED operands the result is at fp32
accumulation level; against the unrounded product it is what 11-bit operands allow and clearly worse than two planes; the default mode is
untouched; a small DNN trains alike in both modes."""
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ONE_PLANE_TILES = (404, 408, 411)            # gemm_s16_glds 32x64 / 64x128 / 128x128 reading one plane
TWO_PLANE_TILES = (304, 308, 311, 328, 351)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def default_mode_afterwards(aslp):
    yield
    aslp.lib.aslp_gemm_operand_planes(-1)
    aslp.lib.aslp_gemm_split16(-1)
    aslp.lib.aslp_gemm_split16_tile(-1)


def s16_exponent(bound):
    """csrc/split16.h s16_exponent"""
    if not (bound > 0.0 and bound < 3.0e38):
        return 0
    return max(-120, min(120, 14 - math.frexp(bound)[1]))


def rounded(X):
    """X16 as float64: fp16(X 2^up) 2^-up with up from the largest finite |x|"""
    a = X.abs()
    up = s16_exponent(a[torch.isfinite(a)].max().item())
    return (X.double() * 2.0 ** up).half().double() * 2.0 ** -up


def product(aslp, planes, tA, tB, A, B):
    C = torch.zeros((A.shape[1] if tA else A.shape[0]), (B.shape[0] if tB else B.shape[1]), device=A.device)
    with aslp.ops.operand_planes(planes):
        aslp.ops.sgemm(tA, tB, 1.0, A, B, 0.0, C)
    return C, aslp.lib.aslp_gemm_last_tile()


def rel_to_abs_product(C, opA, opB):
    return ((C.double() - opA @ opB).abs() / (opA.abs() @ opB.abs())).max().item()


SHAPES = [(0, 1, 1024, 2048, 2048), (0, 0, 1024, 2048, 2048), (1, 0, 2048, 2048, 1024), (1, 1, 512, 640, 768), (0, 1, 1000, 3000, 440),
          (1, 0, 3000, 2048, 1024), (0, 0, 132, 260, 68), (1, 0, 436, 128, 2052), (0, 1, 256, 2048, 2048), (0, 0, 256, 2048, 3000),
          (0, 1, 192, 1920, 1028)]   # (tests/test_gemm_split16_gpu.py's: four layouts, ragged sizes, minibatch 256 = K split over workgroups)


@pytest.mark.parametrize("tA,tB,M,N,K", SHAPES)
def test_exact_operand_model_and_one_plane_error(aslp, dev, tA, tB, M, N, K):
    g = torch.Generator(device=dev).manual_seed(M + 3 * N + 7 * K)
    A = torch.randn((K, M) if tA else (M, K), device=dev, generator=g)
    B = torch.randn((N, K) if tB else (K, N), device=dev, generator=g)
    c1, tile1 = product(aslp, 1, tA, tB, A, B)
    c2, tile2 = product(aslp, 2, tA, tB, A, B)
    assert tile1 in ONE_PLANE_TILES and tile2 in TWO_PLANE_TILES, (tile1, tile2)
    A16, B16 = rounded(A), rounded(B)
    op = lambda X, t: X.t() if t else X
    # the product of the rounded operands, accumulated in fp32 (measured 0.8-1.5e-7 over these shapes)
    e_model = rel_to_abs_product(c1, op(A16, tA), op(B16, tB))
    assert e_model < 4e-7, e_model
    # against the unrounded product: one plane's operand rounding shows (measured 3.9e-5 ... 2.5e-4, 380-2400 x the two-plane error) and stays
    # under the 11-bit bound 2 * 2^-11 (two factors, each off by at most 2^-12 of the matrix' largest binade ... in practice far below)
    e1 = rel_to_abs_product(c1, op(A.double(), tA), op(B.double(), tB))
    e2 = rel_to_abs_product(c2, op(A.double(), tA), op(B.double(), tB))
    print("model %.3g one-plane %.3g two-plane %.3g" % (e_model, e1, e2))
    assert e1 > 30 * e2, (e1, e2)
    assert e1 < 2 ** -10, e1
    assert not torch.equal(c1, c2)
    again, _ = product(aslp, 1, tA, tB, A, B)
    assert torch.equal(again, c1)      # fixed summation order, no atomics


@pytest.mark.parametrize("sa,sb", [(1e-20, 1.0), (1e-12, 1e8), (1e20, 1e-15), (1.0, 1e-30)])
def test_any_magnitude(aslp, dev, sa, sb):
    """the per-matrix scale takes the magnitude out: tiny gradients neither underflow nor lose more than their 11 bits"""
    g = torch.Generator(device=dev).manual_seed(11)
    A = torch.randn(512, 1024, device=dev, generator=g) * sa
    B = torch.randn(768, 1024, device=dev, generator=g) * sb
    A[5] *= 1e-3          # a row a thousand times smaller than the matrix' largest: still normal in fp16 behind the scale
    c1, tile = product(aslp, 1, 0, 1, A, B)
    assert tile in ONE_PLANE_TILES and torch.isfinite(c1).all()
    assert rel_to_abs_product(c1, rounded(A), rounded(B).t()) < 4e-7
    assert rel_to_abs_product(c1, A.double(), B.double().t()) < 2 ** -10
    assert (c1[5].abs().max() > 0).item()


def test_zero_and_nonfinite_operands(aslp, dev):
    A = torch.zeros(256, 512, device=dev)
    B = torch.randn(384, 512, device=dev)
    c1, tile = product(aslp, 1, 0, 1, A, B)
    assert tile in ONE_PLANE_TILES and (c1 == 0).all()
    A[20:] = torch.randn(236, 512, device=dev)
    A[3, 4] = float("inf")
    A[9, 1] = float("nan")
    c1, _ = product(aslp, 1, 0, 1, A, B)
    assert torch.isnan(c1[9]).all() and not torch.isfinite(c1[3]).any()
    ok = torch.ones(256, dtype=torch.bool, device=dev)
    ok[3] = ok[9] = False
    assert torch.isfinite(c1[ok]).all()
    ref = A[ok].double() @ B.double().t()
    assert ((c1[ok].double() - ref).norm() / ref.norm()).item() < 1e-3
    Bn = B.clone()
    Bn[7, 100] = float("nan")          # a NaN in B poisons its column of C and nothing else
    c1, _ = product(aslp, 1, 0, 1, A, Bn)
    assert torch.isnan(c1[:, 7]).all()
    okc = torch.ones(384, dtype=torch.bool, device=dev)
    okc[7] = False
    assert torch.isfinite(c1[ok][:, okc]).all()


@pytest.mark.parametrize("tA,tB,M,N,K,mmt", [(1, 0, 2048, 2048, 1024, 0.9), (1, 0, 3000, 2048, 1024, 0.0), (0, 1, 2048, 2048, 1024, 0.5),
                                             (0, 1, 256, 2048, 2048, 0.9), (1, 0, 2048, 2048, 256, 0.9)])
def test_full_epilogue(aslp, dev, tA, tB, M, N, K, mmt):
    """momentum on the gradient buffer, clip, W += w_alpha G, column sums with the bias step: the fp32 formulas of the two-plane epilogue applied
    to the one-plane product (column sums of a transposed A: those of A16, the operand the kernel reads)"""
    g = torch.Generator(device=dev).manual_seed(M + N + K)
    A = torch.randn((K, M) if tA else (M, K), device=dev, generator=g)
    B = torch.randn((N, K) if tB else (K, N), device=dev, generator=g)
    G0 = torch.randn(M, N, device=dev, generator=g)
    W0 = torch.randn(M, N, device=dev, generator=g)
    bc0, b0 = torch.randn(M, device=dev, generator=g), torch.randn(M, device=dev, generator=g)
    clip, lr = 60.0, -0.01
    Gd, Wd, bc, b = G0.clone(), W0.clone(), bc0.clone(), b0.clone()
    ep = (aslp._lib.GemmEpilogue(None, clip, Wd.data_ptr(), N, lr, None, 0, 0, bc.data_ptr(), 0.9, b.data_ptr(), -0.02) if tA else
          aslp._lib.GemmEpilogue(None, clip, Wd.data_ptr(), N, lr, None, 0, 0))
    with aslp.ops.operand_planes(1):
        aslp.ops.sgemm(tA, tB, 1.0, A, B, mmt, Gd, ep)
    assert aslp.lib.aslp_gemm_last_tile() in ONE_PLANE_TILES
    A16, B16 = rounded(A), rounded(B)
    Gref = ((A16.t() if tA else A16) @ (B16.t() if tB else B16) + mmt * G0.double()).clamp(-clip, clip)
    rel = lambda x, r: ((x.double() - r).norm() / r.norm()).item()
    assert rel(Gd, Gref) < 2e-6 and rel(Wd, W0.double() + lr * Gref) < 2e-6
    if tA:
        bc_ref = A16.sum(0) + 0.9 * bc0.double()
        assert rel(bc, bc_ref) < 2e-6 and rel(b, b0.double() - 0.02 * bc_ref) < 2e-6


def _split_planes(X, bound):
    """csrc/split16.h s16_split of every element behind the scale of `bound` (fp32 arithmetic; the scale is a power of two)"""
    y = X * (2.0 ** s16_exponent(bound))
    hi = y.half()
    return hi, ((y - hi.float()) * 2048.0).half()


def _extras(aslp, dev, rows, cols, bound):
    """output planes (as a producer kernel takes them) and per-workgroup maxima for an epilogue"""
    hi, lo = (torch.full((rows, cols), 7.0, dtype=torch.float16, device=dev) for _ in range(2))
    slot = torch.tensor([bound], dtype=torch.float32, device=dev)
    wmax, cmax = (torch.full((4096,), -1.0, device=dev) for _ in range(2))
    out = aslp._lib.PlanesOut(hi.data_ptr(), lo.data_ptr(), cols, slot.data_ptr(), None, 0, 0)
    return hi, lo, slot, wmax, cmax, out


@pytest.mark.parametrize("planes,tiles", [(1, (408,)), (2, (308, 328))])
def test_weight_gradient_epilogue_leaves_planes_and_maxima(aslp, dev, planes, tiles):
    """the cfg2 weight-gradient launch (both operands reduction-major, 64 x 128 tile with the EXTRA epilogue): momentum, clip, W += w_alpha C,
    bias gradient and bias step, the planes of the updated W (planes_of = 1) and the maxima of |W| and |C| -- in either mode the fp32 side
    effects are the same formulas applied to the mode's own C, bit for bit where the formula is a rounding of a stored value"""
    M, N, K, mmt, clip, lr = 2048, 2048, 1024, 0.9, 60.0, -0.01
    g = torch.Generator(device=dev).manual_seed(21)
    A, B = torch.randn(K, M, device=dev, generator=g), torch.randn(K, N, device=dev, generator=g)
    G0, W0 = torch.randn(M, N, device=dev, generator=g), torch.randn(M, N, device=dev, generator=g)
    bc0, b0 = torch.randn(M, device=dev, generator=g), torch.randn(M, device=dev, generator=g)
    Gd, Wd, bc, b = G0.clone(), W0.clone(), bc0.clone(), b0.clone()
    bound = W0.abs().max().item() + abs(lr) * clip
    hi, lo, slot, wmax, cmax, out = _extras(aslp, dev, M, N, bound)
    ep = aslp._lib.GemmEpilogue(None, clip, Wd.data_ptr(), N, lr, None, 0, 0, bc.data_ptr(), 0.9, b.data_ptr(), -0.02, None, 0, None, 0,
                                out, 1, wmax.data_ptr(), cmax.data_ptr(), None, None, 0)
    with aslp.ops.operand_planes(planes):
        aslp.ops.sgemm(1, 0, 1.0, A, B, mmt, Gd, ep)
    n = aslp.lib.aslp_gemm_last_parts()
    assert aslp.lib.aslp_gemm_last_tile() in tiles and n > 0, (aslp.lib.aslp_gemm_last_tile(), n)
    opA, opB = (rounded(A), rounded(B)) if planes == 1 else (A.double(), B.double())
    rel = lambda x, r: ((x.double() - r.double()).norm() / r.double().norm()).item()
    assert rel(Gd, (opA.t() @ opB + mmt * G0.double()).clamp(-clip, clip)) < 2e-6
    assert rel(bc, opA.sum(0) + 0.9 * bc0.double()) < 2e-6 and rel(b, b0.double() - 0.02 * bc.double()) < 1e-6
    # W against the stored C: one fp32 multiply-add per element
    assert (Wd - (W0 + lr * Gd)).abs().max().item() <= 2.0 ** -22 * bound
    # the planes are the split of the stored W behind the given bound; the maxima are those of the stored matrices
    h_ref, l_ref = _split_planes(Wd, bound)
    assert torch.equal(hi, h_ref) and torch.equal(lo, l_ref)
    assert wmax[:n].max().item() == Wd.abs().max().item() and cmax[:n].max().item() == Gd.abs().max().item()
    assert (wmax[n:] == -1.0).all() and (cmax[n:] == -1.0).all()


@pytest.mark.parametrize("planes,tiles", [(1, (408,)), (2, (308,))])
def test_forward_and_in_diff_epilogues_with_extras(aslp, dev, planes, tiles):
    """forward product with bias and a sigmoid output whose planes the epilogue leaves (planes_of = 2, bound 1); in-diff product (B read with
    the transposing load) that leaves the maxima of |C|"""
    M, N, K = 1024, 2048, 2048
    g = torch.Generator(device=dev).manual_seed(22)
    x, W = torch.randn(M, K, device=dev, generator=g), torch.randn(N, K, device=dev, generator=g) * 0.03
    bias = torch.randn(N, device=dev, generator=g)
    Cm, act = torch.zeros(M, N, device=dev), torch.zeros(M, N, device=dev)
    hi, lo, slot, wmax, cmax, out = _extras(aslp, dev, M, N, 1.0)
    ep = aslp._lib.GemmEpilogue(bias.data_ptr(), 0.0, None, 0, 0.0, act.data_ptr(), N, 1, None, 0.0, None, 0.0, None, 0, None, 0,
                                out, 2, None, cmax.data_ptr(), None, None, 0)
    with aslp.ops.operand_planes(planes):
        aslp.ops.sgemm(0, 1, 1.0, x, W, 0.0, Cm, ep)
    n = aslp.lib.aslp_gemm_last_parts()
    assert aslp.lib.aslp_gemm_last_tile() in tiles and n > 0, (aslp.lib.aslp_gemm_last_tile(), n)
    opA, opB = (rounded(x), rounded(W)) if planes == 1 else (x.double(), W.double())
    ref = opA @ opB.t() + bias.double()
    assert ((Cm.double() - ref).norm() / ref.norm()).item() < 2e-6
    assert (act - torch.sigmoid(Cm)).abs().max().item() < 5e-6
    h_ref, l_ref = _split_planes(act, 1.0)
    assert torch.equal(hi, h_ref) and torch.equal(lo, l_ref)
    assert cmax[:n].max().item() == Cm.abs().max().item()
    # in-diff: dy [M x N] times W [N x K], maxima of the result for the Sigmoid's backward pass
    dy = torch.randn(M, N, device=dev, generator=g) * 1e-3
    Dm = torch.zeros(M, K, device=dev)
    cmax.fill_(-1.0)
    ep = aslp._lib.GemmEpilogue(None, 0.0, None, 0, 0.0, None, 0, 0, None, 0.0, None, 0.0, None, 0, None, 0,
                                aslp._lib.PlanesOut(), 0, None, cmax.data_ptr(), None, None, 0)
    with aslp.ops.operand_planes(planes):
        aslp.ops.sgemm(0, 0, 1.0, dy, W, 0.0, Dm, ep)
    n = aslp.lib.aslp_gemm_last_parts()
    assert aslp.lib.aslp_gemm_last_tile() in tiles and n > 0, (aslp.lib.aslp_gemm_last_tile(), n)
    opA, opB = (rounded(dy), rounded(W)) if planes == 1 else (dy.double(), W.double())
    ref = opA @ opB
    assert ((Dm.double() - ref).norm() / ref.norm()).item() < 2e-6
    assert cmax[:n].max().item() == Dm.abs().max().item()


def _blstm_steps(aslp, dev, planes):
    """two chunks of a latency-controlled BLSTM whose batched products go out as pairs from prepared planes (tests/test_ab_switches_gpu.py's
    sizes: every product is served by the split path)"""
    S, chunk, T, D = 32, 5, 8, 64
    proto = "<NnetProto>\n<BLstmProjectedStreamsLC> <InputDim> %d <OutputDim> 128 <CellDim> 128 <ParamScale> 0.05 <ClipGradient> 5.0\n</NnetProto>\n" % D
    g = torch.Generator(device="cpu").manual_seed(3)
    outs = []
    aslp.lib.aslp_gemm_profile_reset()
    with aslp.ops.operand_planes(planes):
        net = aslp.Nnet.Init(proto, seed=5)
        net.SetTrainOptions(learn_rate=1e-3, momentum=0.9)
        net.SetChunkSize(chunk)
        for step in range(2):
            x = torch.randn(T * S, D, generator=g).to(dev)
            od = (torch.randn(T * S, 128, generator=g) * 0.1).to(dev)
            net.ResetLstmStreams([1] * S if step == 0 else [0] * S)
            outs.append(net.Propagate(x).cpu().numpy())
            outs.append(net.Backpropagate(od, want_in_diff=True).cpu().numpy())
        outs.append(np.asarray(net.GetParams(), np.float32))
    # every batched product of this layer is a pair of the two directions (nnet/nnet-recurrent.cpp): the tile that carried most flops per layout
    return outs, [aslp.lib.aslp_gemm_profile_tile(v, None, 0) for v in range(3)]


def test_paired_products_of_a_blstm_follow_the_mode(aslp, dev):
    o2, t2 = _blstm_steps(aslp, dev, 2)
    o1, t1 = _blstm_steps(aslp, dev, 1)
    print("blstm tiles NT / NN / TN: two planes %s one plane %s" % (t2, t1))
    assert t2[0] in TWO_PLANE_TILES and t1[0] in ONE_PLANE_TILES, (t2, t1)      # x -> gates, both directions in one launch
    assert all(t < 300 or t in TWO_PLANE_TILES for t in t2) and all(t < 300 or t in ONE_PLANE_TILES for t in t1), (t2, t1)
    gaps = []
    for a, b in zip(o1, o2):
        assert np.isfinite(a).all()
        gaps.append(np.linalg.norm(a - b) / np.linalg.norm(b))
    print("blstm gaps (out, in_diff, out, in_diff, params) " + " ".join("%.3g" % v for v in gaps))
    assert not np.array_equal(o1[0], o2[0])                  # the batched products really lost their lo planes
    assert max(gaps) < 5e-3, gaps                            # 11-bit operands in the batched products, two pieces inside the recurrence


def test_one_plane_tiles_by_number_form_the_same_bits(aslp, dev):
    """404 / 408 / 411 asked for by number (aslp_gemm_split16_tile, by the one-plane or the two-plane number) run and agree bit for bit: every
    tile steps through K in the same order.  The heuristic takes 128 x 128 from 512 such tiles on (measured; csrc/gemm_split16.hip)."""
    g = torch.Generator(device=dev).manual_seed(17)
    A, B = torch.randn(2048, 1024, device=dev, generator=g), torch.randn(2048, 1024, device=dev, generator=g)
    out = {}
    for ask, want in ((404, 404), (408, 408), (411, 411), (304, 404), (311, 411), (0, 408)):
        aslp.lib.aslp_gemm_split16_tile(ask)
        out[ask], tile = product(aslp, 1, 0, 1, A, B)
        assert tile == want, (ask, tile)
        assert torch.equal(out[ask], out[404]), ask
    aslp.lib.aslp_gemm_split16_tile(-1)
    big_a, big_b = torch.randn(4096, 256, device=dev, generator=g), torch.randn(4096, 256, device=dev, generator=g)
    _, tile = product(aslp, 1, 0, 1, big_a, big_b)
    assert tile == 411, tile
    aslp.lib.aslp_gemm_split16_tile(411)                 # a one-plane number in two-plane mode never reports a one-plane tile
    _, tile = product(aslp, 2, 0, 1, A, B)
    assert tile not in ONE_PLANE_TILES, tile


def test_prepared_planes_serve_both_modes(aslp, dev):
    """one aslp.ops.Planes per tensor serves NT, NN and TN products in either mode: the producers write both planes whatever the mode"""
    M, N, K = 1024, 2048, 1024
    g = torch.Generator(device=dev).manual_seed(9)
    x = torch.randn(M, K, device=dev, generator=g)
    W = torch.randn(N, K, device=dev, generator=g) * 0.05
    dy = torch.randn(M, N, device=dev, generator=g) * 1e-3
    px, pW, pdy = aslp.ops.Planes(x), aslp.ops.Planes(W), aslp.ops.Planes(dy)
    for tA, tB, A, pa, B, pb, shape in ((0, 1, x, px, W, pW, (M, N)), (0, 0, dy, pdy, W, pW, (M, K)), (1, 0, dy, pdy, x, px, (N, K))):
        out = {}
        for planes in (1, 2, 1):
            C = torch.zeros(shape, device=dev)
            with aslp.ops.operand_planes(planes):
                aslp.ops.sgemm_planes(tA, tB, 1.0, A, pa, B, pb, 0.0, C)
            assert aslp.lib.aslp_gemm_last_tile() in (ONE_PLANE_TILES if planes == 1 else TWO_PLANE_TILES)
            if planes in out:
                assert torch.equal(out[planes], C)
            out[planes] = C
            own, _ = product(aslp, planes, tA, tB, A, B)      # the call that converts its operands itself
            assert torch.equal(own, C), (tA, tB, planes)
        assert not torch.equal(out[1], out[2])


def test_default_untouched(aslp, dev):
    """a fresh process: never set, set(2), set(1) then set(-1) -- the same bits from a two-plane tile every time"""
    code = r"""
import sys, torch
sys.path.insert(0, %r)
import aslp_import
aslp = aslp_import.load()
aslp.ops.use_torch_stream()
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(1)
A = torch.randn(1024, 2048, device=dev, generator=g); B = torch.randn(2048, 2048, device=dev, generator=g)
def run():
    C = torch.zeros(1024, 2048, device=dev)
    aslp.ops.sgemm(0, 1, 1.0, A, B, 0.0, C)
    assert aslp.lib.aslp_gemm_last_tile() in (304, 308, 311, 328, 351), aslp.lib.aslp_gemm_last_tile()
    return C
assert aslp.lib.aslp_gemm_operand_planes_get() == 2
c0 = run()
aslp.ops.set_operand_planes(2); c1 = run()
aslp.ops.set_operand_planes(1); aslp.ops.set_operand_planes(-1); c2 = run()
assert torch.equal(c0, c1) and torch.equal(c0, c2)
aslp.lib.aslp_gemm_split16(0)       # the fp32 instruction wins over the plane count
aslp.ops.set_operand_planes(1); run_tile = None
C = torch.zeros(1024, 2048, device=dev); aslp.ops.sgemm(0, 1, 1.0, A, B, 0.0, C)
assert aslp.lib.aslp_gemm_last_tile() < 300, aslp.lib.aslp_gemm_last_tile()
torch.cuda.synchronize()
print("default-ok")
""" % ROOT
    env = {k: v for k, v in os.environ.items() if k != "ASLP_GEMM_PLANES"}
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "default-ok" in r.stdout, (r.returncode, r.stdout[-400:], r.stderr[-800:])


def _proto(bn):
    proto, d = "<NnetProto>\n", 440
    for _ in range(3):
        proto += "<AffineTransform> <InputDim> %d <OutputDim> 512 <BiasMean> -2.0 <BiasRange> 4.0 <ParamStddev> 0.05\n" % d
        if bn:
            proto += "<BatchNormalization> <InputDim> 512 <OutputDim> 512\n"
        proto += "<Sigmoid> <InputDim> 512 <OutputDim> 512\n"
        d = 512
    return proto + ("<AffineTransform> <InputDim> 512 <OutputDim> 300 <BiasMean> 0.0 <BiasRange> 0.0 <ParamStddev> 0.05\n"
                    "<Softmax> <InputDim> 300 <OutputDim> 300\n</NnetProto>\n")


def _train(aslp, dev, planes, bn, mmt, steps=50, mb=256):
    """a learnable task: the label is the arg-max of a fixed random projection of the input"""
    g = torch.Generator(device="cpu").manual_seed(5)
    P = torch.randn(440, 300, generator=g)
    with aslp.ops.operand_planes(planes):
        net = aslp.Nnet.Init(_proto(bn), seed=3)
        net.SetTrainOptions(learn_rate=0.008, momentum=mmt)
        losses, acc = [], 0.0
        for step in range(steps):
            x = torch.randn(mb, 440, generator=g)
            lab = (x @ P).argmax(1).to(torch.int32)
            xe = aslp.Xent()
            net.TrainStepXent(xe, x.to(dev), lab.to(dev))
            st = xe.GetStats()
            losses.append((st["loss"] - st["entropy"]) / st["frames"])
            # the step's latest product (a weight gradient) ran on a tile of the mode in force: the engine's products follow the switch
            assert aslp.lib.aslp_gemm_last_tile() in (ONE_PLANE_TILES if planes == 1 else TWO_PLANE_TILES), aslp.lib.aslp_gemm_last_tile()
        x = torch.randn(4 * mb, 440, generator=g)          # frame accuracy on frames the net has not seen
        acc = (net.Propagate(x.to(dev)).argmax(1).cpu() == (x @ P).argmax(1)).float().mean().item()
        params = np.asarray(net.GetParams(), np.float32)
    return np.asarray(losses), acc, params


@pytest.mark.parametrize("bn,mmt", [(False, 0.0), (True, 0.9)])
def test_training_agrees_between_the_modes(aslp, dev, bn, mmt):
    l2, acc2, p2 = _train(aslp, dev, 2, bn, mmt)
    l1, acc1, p1 = _train(aslp, dev, 1, bn, mmt)
    assert np.isfinite(p1).all() and np.isfinite(l1).all()
    assert np.isfinite(l2).all()
    gap = np.abs(l1 - l2).max() / np.abs(l2).max()
    pgap = np.linalg.norm(p1 - p2) / np.linalg.norm(p2)
    print("loss gap %.3g parameter gap %.3g accuracies %.4f %.4f" % (gap, pgap, acc1, acc2))
    assert pgap < 1e-2, pgap
    assert gap < (3.5e-3 if bn else 1e-5), gap                                  # measured 2.6e-6 (momentum 0) and 9.7e-4 (BatchNormalization, momentum 0.9)
    assert abs(acc1 - acc2) <= 0.01, (acc1, acc2)


def test_two_steps_against_the_cpu_oracle(aslp, dev, oracle):
    """smoke()'s comparison at sizes the split path serves, in one-plane mode: outputs after two training steps against the fp32 CPU oracle"""
    import ctypes as C
    import nnet_io
    in_dim, hid, nh, out_dim, mb = 440, 512, 3, 300, 256
    d = oracle.lib.orc_dnn_create(in_dim, hid, nh, out_dim, 1, mb, 11)
    layers, L = [], oracle.lib.orc_dnn_num_layers(d)
    for l in range(L):
        r, c = C.c_int(), C.c_int()
        wp = oracle.lib.orc_dnn_weight(d, l, C.byref(r), C.byref(c))
        W = np.ctypeslib.as_array(wp, shape=(r.value, c.value)).copy()
        b = np.ctypeslib.as_array(oracle.lib.orc_dnn_bias(d, l), shape=(r.value,)).copy()
        layers.append(("<AffineTransform>", c.value, r.value, nnet_io.affine(W, b)))
        if l < L - 1:
            layers.append(("<BatchNormalization>", r.value, r.value, nnet_io.batchnorm(np.zeros(r.value), np.ones(r.value))))
            layers.append(("<Sigmoid>", r.value, r.value, b""))
    layers.append(("<Softmax>", out_dim, out_dim, b""))
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "one_plane.nnet")
        nnet_io.write_simple_nnet(path, layers)
        net = aslp.Nnet.Read(path)
    net.SetTrainOptions(learn_rate=0.002, momentum=0.9)
    xent = aslp.Xent()
    rng = np.random.default_rng(0)
    with aslp.ops.operand_planes(1):
        for step in range(2):
            x = rng.standard_normal((mb, in_dim)).astype(np.float32)
            lab = rng.integers(0, out_dim, mb).astype(np.int32)
            oracle.lib.orc_dnn_train_step(d, x, lab, 0.002, 0.9)
            net.TrainStepXent(xent, torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev))
        out = net.ComponentOutput(net.NumComponents() - 1, mb, out_dim)
    out_ref = np.ctypeslib.as_array(oracle.lib.orc_dnn_output(d), shape=(mb, out_dim))
    err = oracle.rel_err(out, out_ref)
    print("oracle rel err %.3g" % err)
    assert 1e-6 < err < 5e-3, err          # measured 2.3e-4


def test_environment_variable_in_a_child_process(aslp, dev):
    code = r"""
import sys, torch
sys.path.insert(0, %r)
import aslp_import
aslp = aslp_import.load()
aslp.ops.use_torch_stream()
dev = torch.device("cuda:0")
assert aslp.lib.aslp_gemm_operand_planes_get() == 1
A = torch.randn(1024, 2048, device=dev); B = torch.randn(2048, 2048, device=dev); C = torch.zeros(1024, 2048, device=dev)
aslp.ops.sgemm(0, 1, 1.0, A, B, 0.0, C)
assert aslp.lib.aslp_gemm_last_tile() in (404, 408, 411), aslp.lib.aslp_gemm_last_tile()
aslp.ops.set_operand_planes(2)
aslp.ops.sgemm(0, 1, 1.0, A, B, 0.0, C)
assert aslp.lib.aslp_gemm_last_tile() in (304, 308, 311, 328, 351)
aslp.ops.set_operand_planes(-1)
assert aslp.lib.aslp_gemm_operand_planes_get() == 1
torch.cuda.synchronize()
print("env-ok")
""" % ROOT
    env = dict(os.environ, ASLP_GEMM_PLANES="1")
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "env-ok" in r.stdout, (r.returncode, r.stdout[-400:], r.stderr[-800:])
