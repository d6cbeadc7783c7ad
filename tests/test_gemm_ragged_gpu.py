"""Split-fp16 layer products at sizes that are no multiple of 4 (aslp_gemm_split16_ragged / ASLP_GEMM_S16_RAGGED=1, off by default;
csrc/gemm_split16.hip): the number of pdfs of a tree, a 39 x 11 input, an utterance's frame count.  The product kernels are the ones
that serve multiples of 4 -- planes padded to 64 with zeros, the element-wise epilogue -- so the bars are theirs: 2.5e-7 of sum |a||b|
against float64 with two planes, 4e-7 against the product of the rounded operands with one.  What is new is the conversion side, so
every matrix here lives in storage whose rows are longer than the matrix (leading dimensions stay multiples of 4) with NaN behind the last
column: a float read from there shows in the result.  With the switch off nothing changes, and shapes that are multiples of 4 keep their
bits with it on."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import nnet_io

pytestmark = pytest.mark.gpu
TWO_PLANE_TILES = (304, 308, 311, 328, 351)
ONE_PLANE_TILES = (404, 408, 411)
LAYOUTS = [(0, 1), (0, 0), (1, 0), (1, 1)]
# one extent ragged at a time; then every residue 1-3, one column / row / k past a tile edge and one short of it
RAGGED = [(131, 128, 64), (128, 131, 64), (128, 128, 67), (129, 131, 67), (130, 257, 127), (191, 129, 65), (259, 261, 131)]
TOL = 1e-4    # tests/test_nnet_gpu.py's bound against the CPU oracle chain


@pytest.fixture(autouse=True)
def switches_back_afterwards(aslp):
    yield
    aslp.lib.aslp_gemm_split16_ragged(-1)
    aslp.lib.aslp_gemm_operand_planes(-1)
    aslp.lib.aslp_gemm_split16(-1)
    aslp.lib.aslp_gemm_split16_tile(-1)


def padded(values, fill=float("nan"), extra=4):
    """`values` [rows x cols] as a view of storage whose rows are cols rounded up to 4 plus `extra` floats long, `fill` behind column cols"""
    rows, cols = values.shape
    store = torch.full((rows, (cols + 3) // 4 * 4 + extra), fill, device=values.device, dtype=values.dtype)
    store[:, :cols] = values
    return store[:, :cols]


def operands(dev, tA, tB, M, N, K, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed + M + 3 * N + 7 * K)
    A = padded(torch.randn((K, M) if tA else (M, K), device=dev, generator=g))
    B = padded(torch.randn((N, K) if tB else (K, N), device=dev, generator=g))
    return A, B


def output(dev, M, N):
    store = torch.full((M, (N + 3) // 4 * 4 + 4), 7.0, device=dev)
    return store, store[:, :N]


def op(X, t):
    return X.t() if t else X


def err_vs(Cm, opA, opB):
    return ((Cm.double() - opA @ opB).abs() / (opA.abs() @ opB.abs())).max().item()


def s16_exponent(bound):
    if not (bound > 0.0 and bound < 3.0e38):
        return 0
    return max(-120, min(120, 14 - math.frexp(bound)[1]))


def rounded(X):
    """tests/test_gemm_f16_plane_gpu.py's model of a one-plane operand: fp16(X 2^up) 2^-up as float64, up from the largest finite |x|"""
    a = X.abs()
    up = s16_exponent(a[torch.isfinite(a)].max().item())
    return (X.double() * 2.0 ** up).half().double() * 2.0 ** -up


def check_product(aslp, planes, tA, tB, A, B, Cm, tiles=None):
    """the issue's bars for a finished product in `planes`-plane mode; returns the error for the log"""
    tile = aslp.lib.aslp_gemm_last_tile()
    assert tile in (tiles if tiles else (TWO_PLANE_TILES if planes == 2 else ONE_PLANE_TILES)), (planes, tile)
    if planes == 2:
        e = err_vs(Cm, op(A.double(), tA), op(B.double(), tB))
        print("two planes tile %d err %.3g" % (tile, e))
        assert e <= 2.5e-7, e
    else:
        e = err_vs(Cm, op(rounded(A), tA), op(rounded(B), tB))
        print("one plane tile %d err against the rounded operands %.3g" % (tile, e))
        assert e < 4e-7, e
    return e


def untouched(store, N):
    return bool((store[:, N:] == 7.0).all())


# ---- 1. every layout at the smallest ragged sizes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", RAGGED)
@pytest.mark.parametrize("tA,tB", LAYOUTS)
def test_every_layout_against_float64(aslp, dev, tA, tB, M, N, K):
    A, B = operands(dev, tA, tB, M, N, K)
    aslp.lib.aslp_gemm_split16_ragged(1)
    for planes in (2, 1):
        with aslp.ops.operand_planes(planes):
            store, Cm = output(dev, M, N)
            aslp.ops.sgemm(tA, tB, 1.0, A, B, 0.0, Cm)
            check_product(aslp, planes, tA, tB, A, B, Cm)
            assert untouched(store, N)
            # the same call again: the same bits (two-level maximum, fixed summation order, no atomics)
            _, again = output(dev, M, N)
            aslp.ops.sgemm(tA, tB, 1.0, A, B, 0.0, again)
            assert torch.equal(again, Cm)
            # planes made beforehand (aslp_planes_convert) against the call that converts inside, and one of each
            pa, pb = aslp.ops.Planes(A), aslp.ops.Planes(B)
            for qa, qb in ((pa, pb), (pa, None), (None, pb)):
                _, C2 = output(dev, M, N)
                aslp.ops.sgemm_planes(tA, tB, 1.0, A, qa, B, qb, 0.0, C2)
                assert aslp.lib.aslp_gemm_last_tile() == (aslp.lib.aslp_gemm_split16_plan(tA, tB, M, N, K, C2.stride(0), None, None, planes, 0, None))
                assert torch.equal(C2, Cm), (planes, qa is not None, qb is not None)
            # ... also on the two-launch conversion (maximum pass + conversion pass) instead of the single launch
            aslp.lib.aslp_coop_convert(0)
            try:
                pa2, pb2 = aslp.ops.Planes(A), aslp.ops.Planes(B)
                _, C3 = output(dev, M, N)
                aslp.ops.sgemm_planes(tA, tB, 1.0, A, pa2, B, pb2, 0.0, C3)
            finally:
                aslp.lib.aslp_coop_convert(1)
            assert torch.equal(C3, Cm), planes


# ---- 2. every kernel family ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tA,tB", LAYOUTS)
def test_every_kernel_family(aslp, dev, tA, tB):
    """tiles asked for by number at 259 x 261 x 131: gemm_s16_glds 32 x 64 / 64 x 128 in every layout, the three 128 x 128 kernels where
    the layout admits them (311 / 312 / 351: both operands reduction-contiguous; 328: both reduction-major)"""
    M, N, K = 259, 261, 131
    A, B = operands(dev, tA, tB, M, N, K)
    aslp.lib.aslp_gemm_split16_ragged(1)
    asks = [(304, 304, 404), (308, 308, 408)]
    if not tA and tB:
        asks += [(311, 351, 411), (312, 311, 411), (351, 351, 411)]     # (311 asked for runs the producer / consumer kernel; 312 is the one-role one)
    if tA and not tB:
        asks += [(328, 328, 408)]                                        # (gemm_s16_ks128 has no one-plane form)
    for planes in (2, 1):
        outs = {}
        for ask, want2, want1 in asks:
            aslp.lib.aslp_gemm_split16_tile(ask)
            want = want2 if planes == 2 else want1
            with aslp.ops.operand_planes(planes):
                assert aslp.lib.aslp_gemm_split16_plan(tA, tB, M, N, K, 268, None, None, planes, ask, None) == want
                store, Cm = output(dev, M, N)
                aslp.ops.sgemm(tA, tB, 1.0, A, B, 0.0, Cm)
                check_product(aslp, planes, tA, tB, A, B, Cm, (want,))
            assert untouched(store, N)
            outs[ask] = Cm
        # every tile steps through K in the same order
        for ask in outs:
            assert torch.equal(outs[ask], outs[304]), (planes, ask)


def test_weight_gradient_of_a_ragged_output_layer_on_the_128_x_128_kernel(aslp, dev):
    """TN 4101 x 2048 x 1024 (4101 pdfs): the heuristic takes gemm_s16_ks128 (328) as for 4104; same bound, the bits of the 64 x 128 tile,
    and the column sums of the transposed A (the bias gradient) from its fragments"""
    M, N, K = 4101, 2048, 1024
    A, B = operands(dev, 1, 0, M, N, K)
    aslp.lib.aslp_gemm_split16_ragged(1)
    outs = {}
    for ask, want in ((-1, 328), (308, 308)):
        aslp.lib.aslp_gemm_split16_tile(ask)
        store, Cm = output(dev, M, N)
        bc = torch.zeros(M, device=dev)
        ep = aslp._lib.GemmEpilogue(None, 0.0, None, 0, 0.0, None, 0, 0, bc.data_ptr(), 0.0, None, 0.0)
        aslp.ops.sgemm(1, 0, 1.0, A, B, 0.0, Cm, ep)
        check_product(aslp, 2, 1, 0, A, B, Cm, (want,))
        assert untouched(store, N)
        ref = A.double().sum(0)
        assert ((bc.double() - ref).norm() / ref.norm()).item() < 2e-6
        outs[want] = (Cm, bc)
    assert torch.equal(outs[328][0], outs[308][0])


def _split_planes(X, bound):
    """csrc/split16.h s16_split of every element behind the scale of `bound` (fp32 arithmetic; the scale is a power of two)"""
    y = X * (2.0 ** s16_exponent(bound))
    hi = y.half()
    return hi, ((y - hi.float()) * 2048.0).half()


@pytest.mark.parametrize("planes,tile", [(2, 328), (1, 408)])
def test_ragged_rows_keep_the_weight_planes_chain(aslp, dev, planes, tile):
    """the weight-gradient launch of a layer with 4101 outputs and 2048 inputs at minibatch 1024: N is a multiple of 4, so the 16-byte epilogue
    runs and leaves the planes of the updated W (4101 rows: ragged rows, whole columns) and the maxima of |W| and |C|, as
    tests/test_gemm_f16_plane_gpu.py checks it at 2048 x 2048 -- here on gemm_s16_ks128's EXTRA form with a last tile row of 5 rows"""
    M, N, K, mmt, clip, lr = 4101, 2048, 1024, 0.9, 60.0, -0.01
    g = torch.Generator(device=dev).manual_seed(23)
    A, B = padded(torch.randn(K, M, device=dev, generator=g)), torch.randn(K, N, device=dev, generator=g)
    G0, W0 = torch.randn(M, N, device=dev, generator=g), torch.randn(M, N, device=dev, generator=g)
    bc0, b0 = torch.randn(M, device=dev, generator=g), torch.randn(M, device=dev, generator=g)
    Gd, Wd, bc, b = G0.clone(), W0.clone(), bc0.clone(), b0.clone()
    bound = W0.abs().max().item() + abs(lr) * clip
    rows_p = (M + 63) // 64 * 64
    hi, lo = (torch.zeros(rows_p, N, dtype=torch.float16, device=dev) for _ in range(2))      # (padding rows: zero, as PlaneSet::Reserve leaves them)
    slot = torch.tensor([bound], dtype=torch.float32, device=dev)
    wmax, cmax = (torch.full((4096,), -1.0, device=dev) for _ in range(2))
    out = aslp._lib.PlanesOut(hi.data_ptr(), lo.data_ptr(), N, slot.data_ptr(), None, 0, 0)
    ep = aslp._lib.GemmEpilogue(None, clip, Wd.data_ptr(), N, lr, None, 0, 0, bc.data_ptr(), 0.9, b.data_ptr(), -0.02, None, 0, None, 0,
                                out, 1, wmax.data_ptr(), cmax.data_ptr(), None, None, 0)
    aslp.lib.aslp_gemm_split16_ragged(1)
    with aslp.ops.operand_planes(planes):
        aslp.ops.sgemm(1, 0, 1.0, A, B, mmt, Gd, ep)
    n = aslp.lib.aslp_gemm_last_parts()
    assert aslp.lib.aslp_gemm_last_tile() == tile and n > 0, (aslp.lib.aslp_gemm_last_tile(), n)
    opA, opB = (rounded(A), rounded(B)) if planes == 1 else (A.double(), B.double())
    rel = lambda x, r: ((x.double() - r.double()).norm() / r.double().norm()).item()
    assert rel(Gd, (opA.t() @ opB + mmt * G0.double()).clamp(-clip, clip)) < 2e-6
    assert rel(bc, opA.sum(0) + 0.9 * bc0.double()) < 2e-6 and rel(b, b0.double() - 0.02 * bc.double()) < 1e-6
    assert (Wd - (W0 + lr * Gd)).abs().max().item() <= 2.0 ** -22 * bound      # one fp32 multiply-add per element of the stored C
    h_ref, l_ref = _split_planes(Wd, bound)
    assert torch.equal(hi[:M], h_ref) and torch.equal(lo[:M], l_ref)
    assert bool((hi[M:] == 0).all()) and bool((lo[M:] == 0).all())               # nothing written behind the last row
    assert wmax[:n].max().item() == Wd.abs().max().item() and cmax[:n].max().item() == Gd.abs().max().item()
    assert (wmax[n:] == -1.0).all() and (cmax[n:] == -1.0).all()


# ---- 3. K split over workgroups -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tA,tB", [(0, 1), (0, 0), (1, 0)])
@pytest.mark.parametrize("M,N,K,cfg", [(1001, 515, 2051, 0), (130, 131, 2051, 308)])
def test_split_reduction(aslp, dev, tA, tB, M, N, K, cfg):
    """shapes whose plan is chunks of K over workgroups and a second launch that adds them (tests/test_gemm_ragged_cpu.py pins the plan)"""
    A, B = operands(dev, tA, tB, M, N, K)
    aslp.lib.aslp_gemm_split16_ragged(1)
    aslp.lib.aslp_gemm_split16_tile(cfg if cfg else -1)
    for planes in (2, 1):
        split = C.c_int(-1)
        tile = aslp.lib.aslp_gemm_split16_plan(tA, tB, M, N, K, (N + 3) // 4 * 4 + 4, None, None, planes, cfg, C.byref(split))
        assert tile == (308 if planes == 2 else 408) and split.value >= 2, (tile, split.value)
        with aslp.ops.operand_planes(planes):
            store, Cm = output(dev, M, N)
            aslp.ops.sgemm(tA, tB, 1.0, A, B, 0.0, Cm)
            check_product(aslp, planes, tA, tB, A, B, Cm, (tile,))
            assert untouched(store, N)
            _, again = output(dev, M, N)
            aslp.ops.sgemm(tA, tB, 1.0, A, B, 0.0, again)
            assert torch.equal(again, Cm)


# ---- 4. nothing outside the matrix is read or written --------------------------------------------------------------------------------
def window(dev, values, fill):
    """`values` as a window of a larger tensor full of `fill`: 3 rows above and below, 4 columns (a multiple of 4) to the left, the rest
    of a longer row to the right"""
    rows, cols = values.shape
    big = torch.full((rows + 6, (cols + 3) // 4 * 4 + 12), fill, device=dev)
    big[3:3 + rows, 4:4 + cols] = values
    return big, big[3:3 + rows, 4:4 + cols]


class Handle:
    """an aslp_planes the test fills through the producer interface (what aslp.ops.Planes is for aslp_planes_convert)"""

    def __init__(self, aslp, rows, cols):
        self.lib = aslp.lib
        self.h = C.c_void_p(self.lib.aslp_planes_new())
        self.lib.aslp_planes_reserve(self.h, rows, cols)

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.aslp_planes_free(self.h)
            self.h = None


@pytest.mark.parametrize("tA,tB", [(0, 1), (1, 0)])
@pytest.mark.parametrize("planes", [2, 1])
def test_nothing_outside_the_matrix_is_read_or_written(aslp, dev, tA, tB, planes):
    """A, B and C as windows of larger tensors.  NaN around A and B would reach a plane, 1e30 would reach the maximum (the scale would move
    and the bits with it): C is bit-identical to the run on copies that stand alone, and C's surroundings keep their 7.0 -- converting
    inside the call, through aslp_planes_convert and through aslp_copy_mat_planes"""
    M, N, K = 129, 131, 67
    lib, ptr, dim = aslp.lib, aslp.ops.ptr, aslp.ops.dim
    g = torch.Generator(device=dev).manual_seed(5 + tA)
    a = torch.randn((K, M) if tA else (M, K), device=dev, generator=g)
    b = torch.randn((N, K) if tB else (K, N), device=dev, generator=g)
    aslp.lib.aslp_gemm_split16_ragged(1)
    with aslp.ops.operand_planes(planes):
        _, ref = output(dev, M, N)
        aslp.ops.sgemm(tA, tB, 1.0, padded(a, 0.0), padded(b, 0.0), 0.0, ref)
        check_product(aslp, planes, tA, tB, a, b, ref)
        for fill in (float("nan"), 1e30):
            _, A = window(dev, a, fill)
            _, B = window(dev, b, fill)

            def run(pa, pb):
                cbig, Cw = window(dev, torch.full((M, N), 7.0, device=dev), 7.0)
                aslp.ops.sgemm_planes(tA, tB, 1.0, A, pa, B, pb, 0.0, Cw)
                assert aslp.lib.aslp_gemm_last_tile() >= 300
                assert torch.equal(Cw, ref), (fill, pa is not None)
                keep = torch.ones_like(cbig, dtype=torch.bool)
                keep[3:3 + M, 4:4 + N] = False
                assert bool((cbig[keep] == 7.0).all()), fill

            run(None, None)
            run(aslp.ops.Planes(A), aslp.ops.Planes(B))
            aslp.lib.aslp_coop_convert(0)       # the maximum pass + conversion pass instead of the single launch
            try:
                pa, pb = aslp.ops.Planes(A), aslp.ops.Planes(B)
            finally:
                aslp.lib.aslp_coop_convert(1)
            run(pa, pb)
            # aslp_copy_mat_planes: the copy goes into a window too
            made = []
            for src in (A, B):
                h = Handle(aslp, src.shape[0], src.shape[1])
                po = aslp._lib.PlanesOut()
                lib.aslp_planes_as_output(h.h, C.byref(po))
                dbig, dst = window(dev, torch.full(src.shape, -7.0, device=dev), -7.0)
                rc = lib.aslp_copy_mat_planes(ptr(dst), dim(dst), ptr(src), dim(src).stride, C.byref(po))
                aslp.ops.check_error()
                torch.cuda.synchronize()
                if rc == 0:     # declined: nothing was written
                    assert po.planes_written == 0 and bool((dbig == -7.0).all())
                    made.append(None)
                    continue
                assert rc == 1 and po.planes_written == 1
                assert torch.equal(dst.contiguous().view(torch.int32), src.contiguous().view(torch.int32))
                keep = torch.ones_like(dbig, dtype=torch.bool)
                keep[3:3 + src.shape[0], 4:4 + src.shape[1]] = False
                assert bool((dbig[keep] == -7.0).all()), fill
                made.append(h)
            run(made[0], made[1])


def test_absmax_parts_of_a_window(aslp, dev):
    """aslp_absmax_parts (the start of the kept-weight-planes chain) at a ragged width: the maxima are the window's own"""
    g = torch.Generator(device=dev).manual_seed(3)
    w = torch.randn(131, 129, device=dev, generator=g)
    parts = torch.full((256,), -1.0, device=dev)
    aslp.lib.aslp_gemm_split16_ragged(1)
    for fill in (1e30, float("nan")):
        _, W = window(dev, w, fill)
        aslp.lib.aslp_absmax_parts(aslp.ops.ptr(W), aslp.ops.dim(W), aslp.ops.ptr(parts))
        aslp.ops.check_error()
        assert parts.max().item() == w.abs().max().item() and parts.min().item() >= 0.0


# ---- 5. full epilogue -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes", [2, 1])
def test_full_epilogue(aslp, dev, planes):
    """the weight-gradient call of a layer with 131 outputs and 129 inputs at minibatch 130: momentum on the gradient buffer, clip,
    W += w_alpha G, the bias gradient from the column sums of the transposed A and the bias step (one plane: the sums of the rounded A)"""
    M, N, K, mmt, clip, lr = 131, 129, 130, 0.9, 60.0, -0.01
    g = torch.Generator(device=dev).manual_seed(M + N + K)
    A, B = padded(torch.randn(K, M, device=dev, generator=g)), padded(torch.randn(K, N, device=dev, generator=g))
    G0, W0 = torch.randn(M, N, device=dev, generator=g), torch.randn(M, N, device=dev, generator=g)
    bc0, b0 = torch.randn(M, device=dev, generator=g), torch.randn(M, device=dev, generator=g)
    Gd, Wd, bc, b = padded(G0, 7.0), padded(W0, 7.0), bc0.clone(), b0.clone()
    ep = aslp._lib.GemmEpilogue(None, clip, Wd.data_ptr(), Wd.stride(0), lr, None, 0, 0, bc.data_ptr(), 0.9, b.data_ptr(), -0.02)
    aslp.lib.aslp_gemm_split16_ragged(1)
    with aslp.ops.operand_planes(planes):
        aslp.ops.sgemm(1, 0, 1.0, A, B, mmt, Gd, ep)
    assert aslp.lib.aslp_gemm_last_tile() in (TWO_PLANE_TILES if planes == 2 else ONE_PLANE_TILES)
    opA, opB = (rounded(A), rounded(B)) if planes == 1 else (A.double(), B.double())
    Gref = (opA.t() @ opB + mmt * G0.double()).clamp(-clip, clip)
    rel = lambda x, r: ((x.double() - r).norm() / r.norm()).item()
    bc_ref = opA.sum(0) + 0.9 * bc0.double()
    errs = (rel(Gd, Gref), rel(Wd, W0.double() + lr * Gref), rel(bc, bc_ref), rel(b, b0.double() - 0.02 * bc_ref))
    print("full epilogue, %d planes: G %.3g W %.3g bias gradient %.3g bias %.3g" % ((planes,) + errs))
    assert max(errs) < 2e-6, errs


# ---- 6. a net ----------------------------------------------------------------------------------------------------------------------
DIMS = (129, 131, 130, 133)      # 129 -> 131 Sigmoid -> 130 Sigmoid -> 133 Softmax
MB, LR, MMT, STEPS = 134, 0.008, 0.9, 3


def _initial_model(seed=7):
    rng = np.random.default_rng(seed)
    return [((rng.standard_normal((o, i)) * 0.1).astype(np.float32), (rng.standard_normal(o) * 0.1).astype(np.float32)) for i, o in zip(DIMS[:-1], DIMS[1:])]


def _batches():
    rng = np.random.default_rng(8)
    return [(rng.standard_normal((MB, DIMS[0])).astype(np.float32), rng.integers(0, DIMS[-1], MB).astype(np.int32)) for _ in range(STEPS)]


@pytest.fixture(scope="module")
def oracle_chain(oracle):
    """the CPU oracle's three steps from the initial model, computed once: per step (posteriors, input's in-diff, parameters after, loss)"""
    layers = [oracle.Affine(W, b) for W, b in _initial_model()]
    ref = []
    for x, lab in _batches():
        h1 = oracle.unary("orc_sigmoid", layers[0].propagate(x))
        h2 = oracle.unary("orc_sigmoid", layers[1].propagate(h1))
        y = oracle.unary("orc_softmax_rows", layers[2].propagate(h2))
        tgt = np.zeros((MB, DIMS[-1]), np.float32)
        tgt[np.arange(MB), lab] = 1
        diff, st = oracle.xent_eval(np.ones(MB, np.float32), y, tgt)
        d2 = oracle.binary("orc_diff_sigmoid", h2, layers[2].backpropagate(diff))
        d1 = oracle.binary("orc_diff_sigmoid", h1, layers[1].backpropagate(d2))
        idf = layers[0].backpropagate(d1)
        for layer, inp, od in ((layers[2], h2, diff), (layers[1], h1, d2), (layers[0], x, d1)):
            layer.update(inp, od, LR, MMT)
        ref.append((y, idf, np.concatenate([np.concatenate([l.W.ravel(), l.b]) for l in layers]), (st["loss"] - st["entropy"]) / st["frames"]))
    return ref


def _engine_steps(aslp, dev, tmp_path):
    """the same three steps on the engine, every buffer the test hands in with a padded pitch: per step (posteriors, in-diff, parameters,
    loss), and the tile that carried most flops per layout (NT forward, NN in-diff, TN weight gradient)"""
    spec = []
    for k, (W, b) in enumerate(_initial_model()):
        spec.append(("<AffineTransform>", W.shape[1], W.shape[0], nnet_io.affine(W, b)))
        spec.append(("<Sigmoid>" if k < 2 else "<Softmax>", W.shape[0], W.shape[0], b""))
    path = tmp_path / "ragged.nnet"
    nnet_io.write_simple_nnet(path, spec)
    net = aslp.Nnet.Read(path)
    net.SetTrainOptions(learn_rate=LR, momentum=MMT)
    got = []
    aslp.lib.aslp_gemm_profile_reset()
    for x, lab in _batches():
        xd = padded(torch.from_numpy(x).to(dev))
        out = padded(torch.zeros(MB, DIMS[-1], device=dev))
        net.Propagate(xd, out=out)
        xe = aslp.Xent()
        diff = padded(torch.zeros(MB, DIMS[-1], device=dev))
        xe.Eval(torch.ones(MB, device=dev), out, diff, labels=torch.from_numpy(lab).to(dev))
        idf = net.Backpropagate(diff, want_in_diff=True)
        st = xe.GetStats()
        got.append((out.cpu().numpy(), idf.cpu().numpy(), net.GetParams(), (st["loss"] - st["entropy"]) / st["frames"]))
    tiles = [aslp.lib.aslp_gemm_profile_tile(v, None, 0) for v in range(3)]
    # flops per layout on the fp32 instruction's tiles, on two-plane and on one-plane tiles (every product of this net is at least 128 x 128 x 64)
    flops = [tuple(aslp.lib.aslp_gemm_profile_tile_flops(v, lo, hi) for lo, hi in ((0, 300), (300, 400), (400, 500))) for v in range(3)]
    return got, tiles, flops


def test_a_net_of_ragged_layers(aslp, oracle, dev, tmp_path, oracle_chain):
    """every product of this net is at least 128 x 128 x 64 and none has a size that is a multiple of 4.  Under the switch they all run on
    split-fp16 tiles; outputs, the input's in-diff and the parameters follow the CPU oracle chain as tests/test_nnet_gpu.py asks of its
    net.  With one plane: one-plane tiles, and the two modes as close as tests/test_gemm_f16_plane_gpu.py's training test asks (parameters
    1e-2; the loss 1e-5, its bound for a net without BatchNormalization -- its 3.5e-3 is for the BatchNormalization run)."""
    want = [sum(2.0 * MB * i * o for i, o in zip(DIMS[:-1], DIMS[1:])) * STEPS] * 3      # forward, in-diff, weight gradient: the same flops
    aslp.lib.aslp_gemm_split16_ragged(0)
    _, tiles_off, flops_off = _engine_steps(aslp, dev, tmp_path)
    assert all(0 < t < 300 for t in tiles_off), tiles_off      # as shipped: the fp32 instruction
    assert [f[0] for f in flops_off] == want and all(f[1] == 0 and f[2] == 0 for f in flops_off), flops_off
    aslp.lib.aslp_gemm_split16_ragged(1)
    got2, tiles2, flops2 = _engine_steps(aslp, dev, tmp_path)
    print("ragged net tiles NT / NN / TN: off %s two planes %s" % (tiles_off, tiles2))
    assert all(t in TWO_PLANE_TILES for t in tiles2), tiles2
    assert [f[1] for f in flops2] == want and all(f[0] == 0 and f[2] == 0 for f in flops2), flops2      # every product, not just most flops
    for step, ((y, idf, par, loss), (y_ref, idf_ref, par_ref, loss_ref)) in enumerate(zip(got2, oracle_chain)):
        for name, a, r in (("output", y, y_ref), ("in_diff", idf, idf_ref), ("params", par, par_ref)):
            rel, mx = oracle.rel_err(a, r), oracle.max_err(a, r)
            print("ragged net step %d %s: rel %.3g max %.3g" % (step, name, rel, mx))
            assert np.isfinite(a).all() and rel < TOL and mx < 10 * TOL, (name, step, rel, mx)
        assert abs(loss - loss_ref) < 1e-5 * abs(loss_ref), (step, loss, loss_ref)
    with aslp.ops.operand_planes(1):
        got1, tiles1, flops1 = _engine_steps(aslp, dev, tmp_path)
    assert all(t in ONE_PLANE_TILES for t in tiles1), tiles1
    assert [f[2] for f in flops1] == want and all(f[0] == 0 and f[1] == 0 for f in flops1), flops1
    pgap = np.linalg.norm(got1[-1][2] - got2[-1][2]) / np.linalg.norm(got2[-1][2])
    lgap = max(abs(a[3] - b[3]) for a, b in zip(got1, got2)) / max(abs(b[3]) for b in got2)
    print("ragged net, one plane against two: parameter gap %.3g loss gap %.3g tiles %s" % (pgap, lgap, tiles1))
    assert all(np.isfinite(g[2]).all() for g in got1)
    assert not np.array_equal(got1[0][0], got2[0][0])        # the products really lost their lo planes
    assert pgap < 1e-2 and lgap < 1e-5, (pgap, lgap)


def test_an_lstm_layer_with_a_ragged_input(aslp, dev):
    """<LstmProjectedStreams> with a 131-wide input (T = 8, S = 16: 128 rows; 128 cells, 64 projected): its batched products with the
    input -- gates, in-diff, the input weights' gradient -- are ragged.  One step with the switch on, one with it off, from one model."""
    T, S, D, R = 8, 16, 131, 64
    proto = "<NnetProto>\n<LstmProjectedStreams> <InputDim> %d <OutputDim> %d <CellDim> 128 <ParamScale> 0.05 <ClipGradient> 5.0\n</NnetProto>\n" % (D, R)
    g = torch.Generator(device="cpu").manual_seed(4)
    x = padded(torch.randn(T * S, D, generator=g).to(dev))
    od = (torch.randn(T * S, R, generator=g) * 0.1).to(dev)
    runs = []
    for on in (1, 0):
        aslp.lib.aslp_gemm_split16_ragged(on)
        aslp.lib.aslp_gemm_profile_reset()
        net = aslp.Nnet.Init(proto, seed=5)
        net.SetTrainOptions(learn_rate=1e-3, momentum=0.9)
        net.ResetLstmStreams([1] * S)
        out = net.Propagate(x).cpu().numpy()
        idf = net.Backpropagate(od, want_in_diff=True).cpu().numpy()
        runs.append((out, idf, np.asarray(net.GetParams(), np.float32), [aslp.lib.aslp_gemm_profile_tile(v, None, 0) for v in range(3)]))
    print("lstm tiles NT / NN / TN: switch on %s off %s" % (runs[0][3], runs[1][3]))
    assert max(runs[0][3]) >= 300        # the ragged products of the layer did move to the split kernels
    for name, a, b in zip(("out", "in_diff", "params"), runs[0], runs[1]):
        assert a.shape == b.shape and np.isfinite(a).all()
        gap = np.linalg.norm(a - b) / np.linalg.norm(b)
        print("lstm %s: switch on against off %.3g" % (name, gap))
        assert gap < 1e-4, (name, gap)


# ---- 7. the default is untouched ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tA,tB", LAYOUTS)
def test_switch_off_ragged_shapes_stay_where_they_were(aslp, dev, tA, tB):
    aslp.lib.aslp_gemm_split16_ragged(0)
    for M, N, K in RAGGED:
        g = torch.Generator(device=dev).manual_seed(M + N + K)
        A = padded(torch.randn((K, M) if tA else (M, K), device=dev, generator=g), 0.0)
        B = padded(torch.randn((N, K) if tB else (K, N), device=dev, generator=g), 0.0)
        outs = []
        for split in (-1, 0):
            aslp.lib.aslp_gemm_split16(split)
            _, Cm = output(dev, M, N)
            aslp.ops.sgemm(tA, tB, 1.0, A, B, 0.0, Cm)
            assert 0 < aslp.lib.aslp_gemm_last_tile() < 300, (M, N, K, aslp.lib.aslp_gemm_last_tile())
            outs.append(Cm)
        assert torch.equal(outs[0], outs[1]), (M, N, K)
        assert aslp.lib.aslp_gemm_split16_plan(tA, tB, M, N, K, N, None, None, 0, 0, None) == 0
    # the conversions refuse such a width as they did
    aslp.lib.aslp_gemm_split16(-1)
    with pytest.raises(ValueError):
        aslp.ops.Planes(padded(torch.zeros(64, 67, device=dev), 0.0))


@pytest.mark.parametrize("tA,tB,M,N,K", [(0, 0, 132, 260, 68), (0, 1, 1000, 3000, 440)])
def test_switch_on_multiples_of_4_keep_their_bits(aslp, dev, tA, tB, M, N, K):
    g = torch.Generator(device=dev).manual_seed(M + N + K)
    A = torch.randn((K, M) if tA else (M, K), device=dev, generator=g)
    B = torch.randn((N, K) if tB else (K, N), device=dev, generator=g)
    for planes in (2, 1):
        res = {}
        with aslp.ops.operand_planes(planes):
            for on in (0, 1):
                aslp.lib.aslp_gemm_split16_ragged(on)
                inside = torch.zeros(M, N, device=dev)
                aslp.ops.sgemm(tA, tB, 1.0, A, B, 0.0, inside)
                tile = aslp.lib.aslp_gemm_last_tile()
                assert tile in (TWO_PLANE_TILES if planes == 2 else ONE_PLANE_TILES)
                prepared = torch.zeros(M, N, device=dev)
                aslp.ops.sgemm_planes(tA, tB, 1.0, A, aslp.ops.Planes(A), B, aslp.ops.Planes(B), 0.0, prepared)
                res[on] = (inside, prepared, tile)
        assert res[0][2] == res[1][2]
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][0], res[0][1]), planes
