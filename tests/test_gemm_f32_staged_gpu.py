"""The register-staged fp32 product kernel (gemm_f32_mfma, csrc/gemm.hip): each of its 24 instantiations -- tiles 1 (32 x 128 x 16),
7 (64 x 64 x 32) and 12 (64 x 128 x 32 on 8 waves) x NT / NN / TN / TT x vector / scalar load path -- asked for by number
(aslp_gemm_force_tile) and checked element by element against float64.

Shapes: the smallest at which the kernel can go wrong -- partial tiles in M and N, M <= 32, and K-tile counts 1 / even / odd > 1 for both
K tiles (16 and 32), with and without a K tail.  (The first five shapes of each path give the 16-deep K tile of tile 1 odd counts only --
1, 3, 5, 7 -- so each path has a sixth with two of them, K = 32 without a tail and K = 30 with one: the round-up-to-even adds no tile.)  The vector path takes 16-byte aligned operands whose rows are a multiple of 4 floats long
and whose extents are multiples of 4; everything else runs the scalar path: odd extents, and aligned extents behind a pointer that is one
float off.  (Which load path ran is not reported by the library; the operands are built to the conditions of launch_aligned.)

Launches per shape: (a) alpha = 1, beta = 0 into a C full of NaN, with bias and a sigmoid act_out; (b) alpha = 0.7, beta = 1.3 with c_src a
column block of a wider matrix; (c) beta = 0.9 with clip, W and w_alpha (the folded SGD step), the clip chosen on the CPU so that the
float64 reference has clipped and unclipped elements (a 1 x 1 product runs (c) twice, once either side of its one element).

C, W and act_out are interior views of larger buffers: nothing outside the view may change.  Bounds, with u = 2^-24, for every element:
|got - ref| <= (K + 4) u (|alpha| (|op A| |op B|) + |beta c| + |bias|) -- K roundings of the accumulation, the epilogue's two, and slack;
clipping is 1-Lipschitz, so the bound survives it.  W: |w_alpha| times that, plus 2 u |W ref|.  act_out: the oracle's sigmoid of the stored
output at 1e-6 (tests/test_kernels_gpu.py::test_sgemm_epilogue).  The relative Frobenius bound 2e-6 of test_sgemm_vs_oracle holds as well.

devtools/gemm_f32_sweep.py imports the case table, host() and launch() and hashes what the same calls write."""
import functools
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TILES = (1, 7, 12)
LAYOUTS = [(0, 1), (0, 0), (1, 0), (1, 1)]      # (transA, transB): NT, NN, TN, TT
Case = namedtuple("Case", "M N K a_off")        # a_off: floats between the start of A's buffer (16-byte aligned) and A
PATHS = {
    "vector": [Case(4, 4, 4, 0), Case(68, 132, 36, 0), Case(36, 260, 68, 0), Case(72, 40, 104, 0), Case(132, 68, 16, 0), Case(36, 132, 32, 0)],
    "scalar": [Case(1, 1, 1, 0), Case(33, 129, 1, 0), Case(67, 131, 37, 0), Case(130, 70, 97, 0), Case(68, 132, 36, 1), Case(35, 67, 30, 0)],
}
LAUNCHES = ("a", "b", "c")
ALPHA_BETA = {"a": (1.0, 0.0), "b": (0.7, 1.3), "c": (1.0, 0.9)}
W_ALPHA = -0.01
FILL = 7.0
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def host(tA, tB, case):
    """inputs of a case from its seed and the float64 references of the three launches, computed once on the CPU and shared by the tiles"""
    M, N, K, _ = case
    rng = np.random.default_rng([M, N, K, tA, tB, case.a_off])
    h = SimpleNamespace()
    h.A = rng.standard_normal((K, M) if tA else (M, K)).astype(np.float32)
    h.B = rng.standard_normal((N, K) if tB else (K, N)).astype(np.float32)
    h.bias = rng.standard_normal(N).astype(np.float32)
    h.wide = rng.standard_normal((M, 2 * N + 4)).astype(np.float32)     # c_src = wide[:, N + 4:]
    h.G0 = rng.standard_normal((M, N)).astype(np.float32)
    h.W0 = rng.standard_normal((M, N)).astype(np.float32)
    opA = (h.A.T if tA else h.A).astype(np.float64)
    opB = (h.B.T if tB else h.B).astype(np.float64)
    P, absP = opA @ opB, np.abs(opA) @ np.abs(opB)
    src = h.wide[:, N + 4:].astype(np.float64)
    h.ref, h.bound = {}, {}
    h.ref["a"], h.bound["a"] = P + h.bias, (K + 4) * U * (absP + np.abs(h.bias.astype(np.float64)))
    h.ref["b"], h.bound["b"] = 0.7 * P + 1.3 * src, (K + 4) * U * (0.7 * absP + np.abs(1.3 * src))
    h.raw_c = P + 0.9 * h.G0.astype(np.float64)                          # launch (c) before the clip
    h.bound["c"] = (K + 4) * U * (absP + np.abs(0.9 * h.G0.astype(np.float64)))
    mag = np.abs(h.raw_c)
    h.clips = tuple(float(np.float32(c)) for c in ((0.5 * mag[0, 0], 2.0 * mag[0, 0]) if mag.size == 1 else (np.median(mag),)))
    for a in (h.A, h.B, h.bias, h.wide, h.G0, h.W0):
        a.setflags(write=False)
    return h


def ref_c(h, clip):
    """launch (c): the clipped product, the weights after the step, and their bounds"""
    G = np.clip(h.raw_c, -clip, clip)
    Wr = h.W0.astype(np.float64) + W_ALPHA * G
    return G, h.bound["c"], Wr, abs(W_ALPHA) * h.bound["c"] + 2 * U * np.abs(Wr)


def operand(dev, values, off=0):
    """`values` in rows a multiple of 4 floats long (+ 4), NaN behind every row's last column, starting `off` floats into its buffer"""
    rows, cols = values.shape
    ld = (cols + 3) // 4 * 4 + 4
    flat = torch.full((rows * ld + 4,), NAN, device=dev)
    view = flat[off:off + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(torch.tensor(values))
    return view


def window(dev, rows, cols, values=None):
    """a rows x cols interior view of a larger buffer full of FILL: 3 rows above and below, 4 columns to the left, 8 or more to the right;
    the view holds `values`, or NaN"""
    big = torch.full((rows + 6, (cols + 3) // 4 * 4 + 12), FILL, device=dev)
    view = big[3:3 + rows, 4:4 + cols]
    if values is None:
        view.fill_(NAN)
    else:
        view.copy_(torch.tensor(values))
    return big, view


def outside_untouched(big, rows, cols):
    keep = torch.ones_like(big, dtype=torch.bool)
    keep[3:3 + rows, 4:4 + cols] = False
    return bool((big[keep] == FILL).all())


def launch(aslp, dev, tile, tA, tB, case, which, clip=0.0):
    """one product of `case` on the forced `tile` -> (the tile the library names, {name: (buffer, view)} of everything the call may write)"""
    h = host(tA, tB, case)
    M, N = case.M, case.N
    Ep = aslp._lib.GemmEpilogue
    A, B = operand(dev, h.A, case.a_off), operand(dev, h.B)
    out = {}
    if which == "a":
        out["C"], out["act"] = window(dev, M, N), window(dev, M, N)
        bias, act = torch.tensor(h.bias).to(dev), out["act"][1]
        ep = Ep(bias.data_ptr(), 0.0, None, 0, 0.0, act.data_ptr(), act.stride(0), 1)
    elif which == "b":
        out["C"] = window(dev, M, N)
        wide = torch.tensor(h.wide).to(dev)
        src = wide[:, N + 4:]            # as tests/test_kernels_gpu.py::test_sgemm_beta_term_from_another_matrix builds it
        ep = Ep(None, 0.0, None, 0, 0.0, None, 0, 0, None, 0.0, None, 0.0, None, 0, src.data_ptr(), wide.stride(0))
    else:
        out["C"], out["W"] = window(dev, M, N, h.G0), window(dev, M, N, h.W0)
        W = out["W"][1]
        ep = Ep(None, clip, W.data_ptr(), W.stride(0), W_ALPHA, None, 0, 0)
    alpha, beta = ALPHA_BETA[which]
    aslp.lib.aslp_gemm_force_tile(tile)
    try:
        aslp.ops.sgemm(tA, tB, alpha, A, B, beta, out["C"][1], ep)
        ran = aslp.lib.aslp_gemm_last_tile()
    finally:
        aslp.lib.aslp_gemm_force_tile(0)
    torch.cuda.synchronize()
    return ran, out


def check(what, got, ref, bound):
    got = got.cpu().numpy().astype(np.float64)
    worst = float(np.max(np.abs(got - ref) / np.maximum(bound, 1e-300)))
    den = np.linalg.norm(ref)
    rel = float(np.linalg.norm(got - ref) / den) if den > 0 else float(np.linalg.norm(got - ref))
    print("%s: largest |got - ref| / bound %.3g, relative Frobenius error %.3g" % (what, worst, rel))
    assert np.isfinite(got).all(), what
    assert worst <= 1.0, (what, worst)
    assert rel < 2e-6, (what, rel)


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("tA,tB", LAYOUTS)
@pytest.mark.parametrize("tile", TILES)
def test_instantiation_against_float64(aslp, oracle, dev, tile, tA, tB, path):
    for case in PATHS[path]:
        h, (M, N, K, _) = host(tA, tB, case), case
        for which in LAUNCHES:
            clipped = unclipped = False
            for clip in (h.clips if which == "c" else (0.0,)):
                what = "tile %d tA %d tB %d %s %s launch %s clip %g" % (tile, tA, tB, path, tuple(case), which, clip)
                ran, out = launch(aslp, dev, tile, tA, tB, case, which, clip)
                assert ran == tile, (what, ran)
                for name, (big, _) in out.items():
                    assert outside_untouched(big, M, N), (what, name)
                if which == "c":
                    G, gb, Wr, wb = ref_c(h, clip)
                    clipped, unclipped = clipped or bool((np.abs(h.raw_c) > clip).any()), unclipped or bool((np.abs(h.raw_c) < clip).any())
                    check(what + " C", out["C"][1], G, gb)
                    check(what + " W", out["W"][1], Wr, wb)
                else:
                    check(what + " C", out["C"][1], h.ref[which], h.bound[which])
                if which == "a":
                    stored = out["C"][1].cpu().numpy()
                    assert oracle.rel_err(out["act"][1].cpu().numpy(), oracle.unary("orc_sigmoid", stored)) < 1e-6, what
            if which == "c":
                assert clipped and unclipped, (tile, tA, tB, tuple(case), h.clips)
