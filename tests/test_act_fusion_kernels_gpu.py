"""Kernels of the Tanh / ReLU fast layer path: the product epilogue's activation output with the per-workgroup maxima of |act_out|
(aslp_gemm_epilogue.amax_parts: the hand-off for an activation without a bound known before the launch) and the backward kernels that
write the in-diff together with its fp16 planes (aslp_diff_relu_p, aslp_diff_tanh_p; aslp_diff_sigmoid_p shares their kernel).  Shapes are
the smallest at which these paths differ: 192 x 320 x 100 is one and a half tile rows, two and a half tile columns and a K that is no
multiple of the K tile; 64 x 64 x 64 is not served by the split-fp16 kernels; 132 rows are no multiple of the 64 the planes are padded to."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def s16_exponent(bound):
    """csrc/split16.h: the scale 2^up puts the bound into [2^13, 2^14); 0, inf and NaN: no scaling"""
    if not (bound > 0.0 and bound < 3.0e38):
        return 0
    return max(-120, min(120, 14 - math.frexp(bound)[1]))


def _epilogue(aslp, **kw):
    ep = aslp._lib.GemmEpilogue()
    for k, v in kw.items():
        setattr(ep, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    return ep


def _act_ref(aslp, Cm, act):
    """the engine's own activation kernels on the stored C: ops.tanh / ReLU as ApplyFloor(0)"""
    ref = Cm.clone()
    if act == 2:
        aslp.ops.tanh(ref, Cm)
    else:
        aslp.lib.cudaF_apply_floor(aslp._lib.D3, aslp._lib.D3, aslp.ops.ptr(ref), 0.0, aslp.ops.dim(ref))
        aslp.ops.check_error()
    return ref


def _bits(t):
    return t.contiguous().view(torch.int32)


def _d2h(aslp, dev_ptr, arr):
    memcpy = aslp.lib.hipMemcpy
    memcpy.restype, memcpy.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    torch.cuda.synchronize()
    assert memcpy(arr.ctypes.data, dev_ptr, arr.nbytes, 2) == 0
    return arr


class _Set:
    """an aslp_planes set whose parts array takes a producer's maxima (what a component's PlaneHolder is to the engine)"""

    def __init__(self, aslp, rows, cols):
        self.lib = aslp.lib
        self.h = C.c_void_p(self.lib.aslp_planes_new())
        self.lib.aslp_planes_reserve(self.h, rows, cols)
        self.po = aslp._lib.PlanesOut()
        self.lib.aslp_planes_as_output(self.h, C.byref(self.po))
        assert self.po.parts and self.po.hi and self.po.slot

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.aslp_planes_free(self.h)
            self.h = None


M, N, K = 192, 320, 100


@pytest.fixture(scope="module")
def operands(dev):
    g = torch.Generator(device=dev).manual_seed(41)
    return (torch.randn(M, K, device=dev, generator=g), torch.randn(N, K, device=dev, generator=g) * 0.2, torch.randn(N, device=dev, generator=g),
            torch.randn(128, N, device=dev, generator=g) * 0.1, torch.randn(128, device=dev, generator=g))


@pytest.mark.parametrize("act", [2, 3])
def test_epilogue_activation_and_its_maxima(aslp, dev, operands, act):
    """act_out is the activation kernel's function of the stored C, bit for bit; for ReLU the per-workgroup maxima are those of act_out (not
    of |C|, which also counts the negative values), exactly, and a conversion that takes them gives the planes of a maximum pass + conversion"""
    x, W, bias, W2, b2 = operands
    Cm, act_out = torch.zeros(M, N, device=dev), torch.full((M, N), 9.0, device=dev)
    ps = _Set(aslp, M, N)
    ep = _epilogue(aslp, bias=bias, act_out=act_out, ld_act=N, act=act, amax_parts=ps.po.parts)
    aslp.lib.aslp_gemm_split16(1)
    try:
        aslp.ops.sgemm(0, 1, 1.0, x, W, 0.0, Cm, ep)
        n = aslp.lib.aslp_gemm_last_parts()
    finally:
        aslp.lib.aslp_gemm_split16(-1)
    ref = x.double() @ W.double().t() + bias.double()
    assert ((Cm.double() - ref).norm() / ref.norm()).item() < 2e-6
    assert torch.equal(_bits(act_out), _bits(_act_ref(aslp, Cm, act)))
    assert n > 0, "the split-fp16 kernel must leave the maxima at this shape"
    parts = _d2h(aslp, ps.po.parts, np.empty(n, np.float32))
    print("act", act, "parts", n, "max part", parts.max(), "max act_out", act_out.abs().max().item(), "max |C|", Cm.abs().max().item())
    assert parts.max() == act_out.abs().max().item()
    if act == 3:
        assert parts.max() == act_out.max().item()
    # the consumer's conversion from these maxima (one streaming launch) ...
    assert aslp.lib.aslp_planes_convert_with_parts(ps.h, aslp.ops.ptr(act_out), aslp.ops.dim(act_out), n) == 0
    aslp.ops.check_error()
    hi = _d2h(aslp, ps.po.hi, np.empty((M, ps.po.ld), np.float16))
    lo = _d2h(aslp, ps.po.lo, np.empty((M, ps.po.ld), np.float16))
    bits = int(_d2h(aslp, ps.po.slot, np.empty(1, np.uint32))[0])
    # ... against the maximum pass + conversion pass of today's consumer: same bound, same planes
    conv = aslp.ops.Planes(act_out)
    cpo = aslp._lib.PlanesOut()
    aslp.lib.aslp_planes_as_output(conv.h, C.byref(cpo))
    assert bits == int(_d2h(aslp, cpo.slot, np.empty(1, np.uint32))[0])
    assert np.array_equal(hi.view(np.uint16), _d2h(aslp, cpo.hi, np.empty((M, cpo.ld), np.float16)).view(np.uint16))
    assert np.array_equal(lo.view(np.uint16), _d2h(aslp, cpo.lo, np.empty((M, cpo.ld), np.float16)).view(np.uint16))


def test_all_negative_product_leaves_zero_maxima_and_finite_planes(aslp, dev, operands):
    """positive A, negative B, negative bias: ReLU's output is all zero and every part is 0 -- the edge at which a scale could become
    infinite.  The conversion leaves zero planes and the next product is exactly its bias."""
    _, _, _, W2, b2 = operands
    g = torch.Generator(device=dev).manual_seed(43)
    x = torch.rand(M, K, device=dev, generator=g) + 0.1
    W = -(torch.rand(N, K, device=dev, generator=g) + 0.1)
    bias = -(torch.rand(N, device=dev, generator=g) + 0.1)
    Cm, act_out = torch.zeros(M, N, device=dev), torch.full((M, N), 9.0, device=dev)
    ps = _Set(aslp, M, N)
    ep = _epilogue(aslp, bias=bias, act_out=act_out, ld_act=N, act=3, amax_parts=ps.po.parts)
    aslp.lib.aslp_gemm_split16(1)
    try:
        aslp.ops.sgemm(0, 1, 1.0, x, W, 0.0, Cm, ep)
        n = aslp.lib.aslp_gemm_last_parts()
        assert n > 0 and Cm.max().item() < 0.0
        assert not act_out.any()
        parts = _d2h(aslp, ps.po.parts, np.empty(n, np.float32))
        assert not parts.any()
        assert aslp.lib.aslp_planes_convert_with_parts(ps.h, aslp.ops.ptr(act_out), aslp.ops.dim(act_out), n) == 0
        aslp.ops.check_error()
        for p in (ps.po.hi, ps.po.lo):
            assert not _d2h(aslp, p, np.empty((M, ps.po.ld), np.float16)).view(np.uint16).any()
        assert np.isfinite(_d2h(aslp, ps.po.slot, np.empty(1, np.float32))[0])
        nxt = torch.full((M, 128), 5.0, device=dev)
        aslp.ops.sgemm_planes(0, 1, 1.0, act_out, ps, W2, None, 0.0, nxt, _epilogue(aslp, bias=b2))
        assert aslp.lib.aslp_gemm_last_tile() >= 300, "the following product must read the planes"
    finally:
        aslp.lib.aslp_gemm_split16(-1)
    assert torch.equal(_bits(nxt), _bits(b2.expand(M, 128)))


@pytest.mark.parametrize("act", [2, 3])
def test_shape_the_split_kernels_do_not_serve_leaves_no_parts(aslp, dev, act):
    g = torch.Generator(device=dev).manual_seed(44)
    x, W, bias = torch.randn(64, 64, device=dev, generator=g), torch.randn(64, 64, device=dev, generator=g), torch.randn(64, device=dev, generator=g)
    Cm, act_out = torch.zeros(64, 64, device=dev), torch.full((64, 64), 9.0, device=dev)
    amax = torch.full((4096,), -1.0, device=dev)
    aslp.ops.sgemm(0, 1, 1.0, x, W, 0.0, Cm, _epilogue(aslp, bias=bias, act_out=act_out, ld_act=64, act=act, amax_parts=amax))
    assert aslp.lib.aslp_gemm_last_parts() == 0
    assert bool((amax == -1.0).all()), "a kernel that cannot leave the parts leaves none"
    ref = x.double() @ W.double().t() + bias.double()
    assert ((Cm.double() - ref).norm() / ref.norm()).item() < 2e-6
    assert torch.equal(_bits(act_out), _bits(_act_ref(aslp, Cm, act)))


# ---- backward kernels that write planes ------------------------------------------------------------------------------------------
def _pad(v):
    return (v + 63) // 64 * 64


def _planes_out(aslp, dev, rows, cols):
    hi, lo = (torch.full((_pad(rows), _pad(cols)), 7.0, dtype=torch.float16, device=dev) for _ in range(2))
    slot = torch.full((1,), float("nan"), device=dev)
    return hi, lo, slot, aslp._lib.PlanesOut(hi.data_ptr(), lo.data_ptr(), _pad(cols), slot.data_ptr(), None, 0, 0)


def _run_p(aslp, kind, out, a, od, parts, po):
    """kind's _p kernel and its plain kernel's result on the same operands (a: the pre-activation for relu, the activation otherwise)"""
    plain = torch.full_like(out, 3.0)
    if kind == "relu":
        rc = aslp.ops.diff_relu_p(out, a, od, parts, po)
        aslp.ops.diff_relu(plain, a, od)
    elif kind == "tanh":
        rc = aslp.ops.diff_tanh_p(out, a, od, parts, po)
        aslp.ops.diff_tanh(plain, a, od)
    else:
        rc = aslp.ops.diff_sigmoid_p(out, a, od, parts, po)
        aslp.ops.diff_sigmoid(plain, a, od)
    return rc, plain


@pytest.mark.parametrize("kind", ["relu", "tanh", "sigmoid"])
@pytest.mark.parametrize("rows,cols", [(192, 320), (132, 128)])
def test_diff_kernels_with_planes(aslp, dev, kind, rows, cols):
    """in-diff bit-identical to the plain kernel; the bound the kernel stores is max |od| (sigmoid: a quarter of it); (hi + 2^-11 lo) / scale
    gives the in-diff back to 2^-22 of the power of two behind the scale (csrc/split16.h: 22 significant bits); nothing outside the matrix
    region of the planes is written."""
    g = torch.Generator(device=dev).manual_seed(rows + cols)
    pre = torch.randn(rows, cols, device=dev, generator=g)
    od = torch.randn(rows, cols, device=dev, generator=g) * 3e-3
    if kind == "relu":
        a = pre.clone()
        a[0, :8] = torch.tensor([0.0, -0.0, 0.0, -0.0, 1e-30, -1e-30, 0.0, -0.0], device=dev)   # zeros of both signs: heaviside is 0 at 0
        od[0, :8] = 1e-3
    else:
        a = torch.tanh(pre) if kind == "tanh" else torch.sigmoid(pre)
    # per-workgroup maxima as a producer leaves them: the matrix maximum somewhere among smaller values
    odmax = od.abs().max().item()
    parts = torch.tensor([0.25 * odmax, 0.0, odmax, 0.5 * odmax, 1e-9], device=dev)
    out = torch.full((rows, cols), 3.0, device=dev)
    hi, lo, slot, po = _planes_out(aslp, dev, rows, cols)
    rc, plain = _run_p(aslp, kind, out, a, od, parts, po)
    assert rc == 1
    assert torch.equal(_bits(out), _bits(plain))
    if kind == "relu":
        assert not out[0, :4].any() and out[0, 4].item() == od[0, 4].item() and out[0, 5].item() == 0.0
    bound = slot.item()
    assert bound == np.float32(0.25 if kind == "sigmoid" else 1.0) * np.float32(odmax)
    assert out.abs().max().item() <= bound
    up = s16_exponent(bound)
    pow2 = 2.0 ** (14 - up)            # the power of two the scale stands for: bound in [pow2 / 2, pow2)
    assert 0.5 * pow2 <= bound < pow2
    rec = (hi[:rows, :cols].double() + lo[:rows, :cols].double() / 2048.0) / 2.0 ** up
    err = (rec - out.double()).abs().max().item()
    print(kind, rows, cols, "bound", bound, "reconstruction error / pow2", err / pow2, "allowed", 2.0 ** -22)
    assert err <= 2.0 ** -22 * pow2
    for p in (hi, lo):   # the padding belongs to whoever reserved the planes
        assert bool((p[rows:] == 7.0).all()) and bool((p[:, cols:] == 7.0).all())


@pytest.mark.parametrize("kind", ["relu", "tanh"])
def test_diff_kernels_zero_out_diff_and_not_served(aslp, dev, kind):
    rows, cols = 132, 128
    g = torch.Generator(device=dev).manual_seed(7)
    a = torch.tanh(torch.randn(rows, cols, device=dev, generator=g))
    od = torch.zeros(rows, cols, device=dev)
    out = torch.full((rows, cols), 3.0, device=dev)
    hi, lo, slot, po = _planes_out(aslp, dev, rows, cols)
    rc, plain = _run_p(aslp, kind, out, a, od, torch.zeros(9, device=dev), po)
    assert rc == 1 and not out.any() and torch.equal(_bits(out), _bits(plain))
    assert math.isfinite(slot.item()) and slot.item() == 0.0
    assert not hi[:rows, :cols].any() and not lo[:rows, :cols].any()
    assert torch.isfinite(hi.float()).all() and torch.isfinite(lo.float()).all()
    # not served (no planes to write to; a view whose rows are not 16-byte aligned): 0, and nothing was launched
    out.fill_(3.0)
    od = torch.randn(rows, cols, device=dev, generator=g)
    fn = aslp.ops.diff_relu_p if kind == "relu" else aslp.ops.diff_tanh_p
    assert fn(out, a, od, torch.ones(4, device=dev), aslp._lib.PlanesOut()) == 0
    wide = torch.randn(rows, cols + 2, device=dev, generator=g)
    assert fn(out, a, wide[:, 1:cols + 1], torch.ones(4, device=dev), po) == 0
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
