"""The temporal filter kernels of csrc/temporal.hip through the C ABI, every path the host rules can pick, element by element against the
float64 models of tests/temporal_ref.py (pinned to the oracle by tests/test_temporal_ref_cpu.py): aslp_rowconv_forward and
aslp_rowconv_backward_fused at every ring length (<4>, <8>, <16>, <21, exact>, <32>) and on the plain kernels (more than 32 taps, one and two
groups of 64 taps, an odd width, an even width with an odd leading dimension on each matrix in turn, a view 4 bytes off an 8-byte boundary),
aslp_rowconv_backward and aslp_rowconv_wgrad on their own on every case, chunk edges of 64 frames (T, L and L + K on either side), streams
past S, an empty stream, ten strips; aslp_fsmn_filter tiled and plain, aslp_fsmn_backward fused and separate, aslp_fsmn_coef_grad on its own,
one-sided filters, the ring block's edge, both staging boundaries, both LDS limits, one, two and three rounds of chunks in the finish, and the
clip.  Every case asks aslp_rowconv_path / aslp_fsmn_path and asserts the path temporal_ref names; the last test asserts all were reached.
The 32-bit offset fallbacks (fsmn_fits32) need buffers of 4 GB and more: out of scope here.

Every case makes two consecutive calls that carry the parameters (and the momentum buffer), once with the folded step and once without (the
parameters must then be untouched bit for bit, and the same inputs give the same gradient bits: a fixed summation order, no atomics).  Matrices
are views with a leading dimension the test chooses, coef and coef_corr with different ones; inputs are padded with NaN, outputs with
SENTINEL, which must still be there afterwards.

The bar is derived in temporal_ref, never measured: |gpu - float64| <= gamma_m A per element, zeros past a stream's length and clipped
elements exact.

MEASURED on an MI355X (for information: the bars are the derived ones and are not adjusted to these figures): the largest err / bar per
group, as test_every_path_was_reached prints it --
    rowconv out 0.77, in_diff 0.99, w_diff 0.49, w_corr 0.22, w 0.22; the plain kernels on their own: in_diff 0.99, w_diff 0.49
    fsmn out 0.61, in_diff 0.66, corr 0.94, coef 0.32; aslp_fsmn_coef_grad on its own 0.94, the reversed filter on its own 0.58
(the ratios near 1 are single products, n = 1: the first frame's in_diff, a tap that meets one frame -- one rounding against a bar of one
rounding; the oracle's own ratios on the same cases are 0.998 and 0.944).  Every case passed as the kernels stood: the second and third
round of fsmn_grad_finish, the step of the separate backward through add_mat, the plain kernels on even widths and the clip in both
finishing kernels compute what the float64 model says.  That the file can tell was tried on a library with five arithmetic changes -- the
finish reading at most 64 chunks, the separate step with lr x 1.001, the fused RowConvolution backward stopping one row early (L + K - 1),
the lower clip of fsmn_coef_grad2 at 0.9999 clip, momentum x 1.0001 in rowconv_wgrad_finish: 20 of the 44 tests failed, each change
in the cases that reach it (d8-p1-f1-t2081 alone; the four cases with C >= 127; every ring case; both clip cases; every ring case).  Of
the five, tests/test_temporal_gpu.py as it stood sees the dropped row (a whole term) and the 1e-3 of the step at 241 taps; it has no case
that reaches the third round of the finish or the clip.
The file takes 2.8 s on the MI355X, 0.9 s of it in the cases; the slowest test is k0-one-frame at 0.27 s (the first launch of the process).
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import temporal_ref as ref

pytestmark = pytest.mark.gpu
SENTINEL = ref.SENTINEL
NAN = float("nan")
_t0 = time.time()
launch_failed = []          # [(what, error)]: once a launch ended in an error, nothing further is started on the GPU
reached = {}                # case -> the paths the library named
worst = {}                  # group -> (largest err / bar, where)
seconds = {}                # test -> seconds


def on_gpu(aslp, what, fn):
    """fn() behind the guard, followed by the library's error check and a synchronize: an error stops every later GPU call of this file"""
    if launch_failed:
        pytest.fail("not started: %s ended in an error, and nothing more runs on the GPU behind it\n%s" % launch_failed[0])
    try:
        out = fn()
        aslp.ops.check_error()
        torch.cuda.synchronize()
        aslp.ops.check_error()
        return out
    except AssertionError:
        raise
    except Exception as e:
        launch_failed.append((what, repr(e)))
        raise


def f32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


class Mat:
    """a [rows x cols] view with leading dimension ld inside a larger buffer: two rows and ld - cols columns of padding, 16 bytes in front;
    offset: the view starts 4 bytes off a 16-byte (and so off an 8-byte) boundary"""

    def __init__(self, dev, rows, cols, ld, fill=None, pad=SENTINEL, offset=False):
        assert ld >= cols
        self.ld, self.pad = ld, pad
        start = 4 + (1 if offset else 0)
        self.buf = torch.full(((rows + 2) * ld + 8,), pad, dtype=torch.float32, device=dev)
        self.v = self.buf[start:start + (rows + 2) * ld].view(rows + 2, ld)[:rows, :cols]
        if fill is not None:
            self.v.copy_(f32(fill, dev))
        self.p = C.c_void_p(self.v.data_ptr())
        assert (self.v.data_ptr() % 16 == 4) == bool(offset)

    def host(self):
        return self.v.cpu().numpy()

    def padding_intact(self):
        keep = self.v.clone()
        self.v.fill_(SENTINEL)
        ok = bool((self.buf == SENTINEL).all())
        self.v.copy_(keep)
        return ok


def vec(dev, a):
    """a dense [D x (K+1)] parameter as the component keeps it, SENTINEL behind it"""
    return Mat(dev, 1, a.size, a.size, a.reshape(1, -1))


def judge(group, what, got, want, fails):
    r = ref.check(got, want, what, fails)
    if not r <= worst.get(group, (-1.0, ""))[0]:
        worst[group] = (r, what)


# ---- RowConvolution -------------------------------------------------------------------------------------------------------------------------
def rc_mats(dev, inp, k):
    c = inp.case
    n = c.T * c.S
    x = Mat(dev, n, c.D, ref.rc_ld(c, "x"), inp.x[k], NAN, offset=c.offset)
    od = Mat(dev, n, c.D, ref.rc_ld(c, "od"), inp.od[k], NAN)
    return x, od


def rc_out(dev, c):
    return Mat(dev, c.T * c.S, c.D, ref.rc_ld(c, "y"))


@pytest.mark.parametrize("name", ref.RC_NAMES)
def test_rowconv_case(aslp, dev, name):
    t0 = time.time()
    inp = ref.rc_inputs(ref.RC_BY_NAME[name])
    c, lib, fails = inp.case, aslp.lib, []
    lens = torch.from_numpy(inp.lens).to(dev)
    lp = C.c_void_p(lens.data_ptr())
    shape = (c.D, c.K + 1)
    want_paths = ref.rc_paths(c)
    for update in (0, 1):
        w, wc = vec(dev, inp.w), vec(dev, inp.w_corr)
        for k in range(2):
            what = "%s update%d call%d" % (name, update, k)
            w0, c0 = w.host().reshape(shape), wc.host().reshape(shape)
            want = ref.rowconv_model(w0, c0, inp.x[k], inp.od[k], c.T, c.S, inp.lens)
            x, od = rc_mats(dev, inp, k)
            out, idf, wd = rc_out(dev, c), rc_out(dev, c), vec(dev, np.full(shape, SENTINEL, np.float32))
            got = (lib.aslp_rowconv_path(c.D, c.K, out.ld, x.ld, 0, out.p, x.p, None), lib.aslp_rowconv_path(c.D, c.K, idf.ld, x.ld, od.ld, idf.p, x.p, od.p))
            assert got == want_paths, (what, got, want_paths)
            on_gpu(aslp, what + " forward", lambda: lib.aslp_rowconv_forward(out.p, out.ld, x.p, x.ld, w.p, c.D, c.K, c.T, c.S, lp))
            judge("rowconv out", what + " out", out.host(), want["out"], fails)
            backward = lambda idf, wd: lib.aslp_rowconv_backward_fused(idf.p, idf.ld, wd.p, x.p, x.ld, od.p, od.ld, w.p, c.D, c.K, c.T, c.S, lp, wc.p,
                                                                     ref.MMT, ref.LR, update)
            on_gpu(aslp, what + " backward", lambda: backward(idf, wd))
            judge("rowconv in_diff", what + " in_diff", idf.host(), want["in_diff"], fails)
            judge("rowconv w_diff", what + " w_diff", wd.host(), want["w_diff"], fails)
            if update:
                judge("rowconv w_corr", what + " w_corr", wc.host(), want["w_corr"], fails)
                judge("rowconv w", what + " w", w.host(), want["w"], fails)
            else:
                assert np.array_equal(w.host().reshape(shape), w0) and np.array_equal(wc.host().reshape(shape), c0), (what, "w / w_corr without a step")
                idf2, wd2 = rc_out(dev, c), vec(dev, np.full(shape, SENTINEL, np.float32))
                on_gpu(aslp, what + " backward again", lambda: backward(idf2, wd2))
                assert torch.equal(idf.buf, idf2.buf) and torch.equal(wd.buf, wd2.buf), (what, "the same inputs, other bits")
                # the plain kernels on their own, whatever the fused entry point picked
                idf3, wd3 = rc_out(dev, c), vec(dev, np.full(shape, SENTINEL, np.float32))
                on_gpu(aslp, what + " plain backward", lambda: lib.aslp_rowconv_backward(idf3.p, idf3.ld, od.p, od.ld, w.p, c.D, c.K, c.T, c.S, lp))
                on_gpu(aslp, what + " plain wgrad", lambda: lib.aslp_rowconv_wgrad(wd3.p, x.p, x.ld, od.p, od.ld, c.D, c.K, c.T, c.S, lp))
                judge("rowconv plain in_diff", what + " plain in_diff", idf3.host(), want["in_diff"], fails)
                judge("rowconv plain w_diff", what + " plain w_diff", wd3.host(), want["w_diff"], fails)
                assert idf3.padding_intact() and wd3.padding_intact(), (what, "padding behind the plain kernels")
            for m, key in ((out, "out"), (idf, "in_diff"), (wd, "w_diff"), (w, "w"), (wc, "w_corr")):
                assert m.padding_intact(), (what, key, "padding")
    reached["rowconv " + name] = want_paths
    seconds["rowconv " + name] = time.time() - t0
    assert not fails, "\n".join(fails)


# ---- CompactFsmn ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.FSMN_NAMES)
def test_fsmn_case(aslp, dev, name):
    t0 = time.time()
    inp = ref.fsmn_inputs(ref.FSMN_BY_NAME[name])
    c, lib, fails = inp.case, aslp.lib, []
    Cn, D, T = c.P + c.F + 1, c.D, c.T
    want_paths = ref.fsmn_paths(c)
    got = (bool(lib.aslp_fsmn_path(D, c.P, c.F, T, D + 5, 0)), bool(lib.aslp_fsmn_path(D, c.P, c.F, T, D + 5, 1)))
    assert got == want_paths, (name, got, want_paths)
    for lr in (0.0, ref.LR):
        coef = Mat(dev, Cn, D, D + 3, inp.coef)
        for k in range(2):
            what = "%s lr%g call%d" % (name, lr, k)
            clip = inp.clip[k]
            coef0 = coef.host()
            want = ref.fsmn_model(coef0, inp.x[k], inp.od[k], c.P, c.F, clip, lr)
            x, od = Mat(dev, T, D, D + 4, inp.x[k], NAN), Mat(dev, T, D, D + 2, inp.od[k], NAN)
            out, idf, corr = Mat(dev, T, D, D + 1), Mat(dev, T, D, D + 5), Mat(dev, Cn, D, D + 1)
            on_gpu(aslp, what + " forward", lambda: lib.aslp_fsmn_filter(out.p, out.ld, x.p, x.ld, coef.p, coef.ld, D, c.P, c.F, T, 0))
            judge("fsmn out", what + " out", out.host(), want["out"], fails)
            backward = lambda idf, corr: lib.aslp_fsmn_backward(idf.p, idf.ld, corr.p, corr.ld, coef.p, coef.ld, x.p, x.ld, od.p, od.ld, D, c.P, c.F, T, clip, lr)
            on_gpu(aslp, what + " backward", lambda: backward(idf, corr))
            judge("fsmn in_diff", what + " in_diff", idf.host(), want["in_diff"], fails)
            judge("fsmn corr", what + " corr", corr.host(), want["corr"], fails)
            if clip > 0.0:
                ref.check_clip(corr.host(), want, clip, what + " corr", fails)
            if lr != 0.0:
                judge("fsmn coef", what + " coef", coef.host(), want["coef"], fails)
            else:
                assert np.array_equal(coef.host(), coef0), (what, "coef without a step")
                idf2, corr2 = Mat(dev, T, D, D + 5), Mat(dev, Cn, D, D + 1)
                on_gpu(aslp, what + " backward again", lambda: backward(idf2, corr2))
                assert torch.equal(idf.buf, idf2.buf) and torch.equal(corr.buf, corr2.buf), (what, "the same inputs, other bits")
                # the tap gradient on its own (the two-stage kernels), and the reversed filter on its own
                corr3, idf3 = Mat(dev, Cn, D, D + 2), Mat(dev, T, D, D + 3)
                on_gpu(aslp, what + " coef_grad", lambda: lib.aslp_fsmn_coef_grad(corr3.p, corr3.ld, x.p, x.ld, od.p, od.ld, D, c.P, c.F, T, clip))
                judge("fsmn coef_grad", what + " coef_grad", corr3.host(), want["corr"], fails)
                if clip > 0.0:
                    ref.check_clip(corr3.host(), want, clip, what + " coef_grad", fails)
                on_gpu(aslp, what + " reversed filter", lambda: lib.aslp_fsmn_filter(idf3.p, idf3.ld, od.p, od.ld, coef.p, coef.ld, D, c.P, c.F, T, 1))
                judge("fsmn reversed filter", what + " reversed filter", idf3.host(), want["in_diff"], fails)
                assert corr3.padding_intact() and idf3.padding_intact(), (what, "padding behind the separate kernels")
            for m, key in ((out, "out"), (idf, "in_diff"), (corr, "corr"), (coef, "coef")):
                assert m.padding_intact(), (what, key, "padding")
    reached["fsmn " + name] = want_paths
    seconds["fsmn " + name] = time.time() - t0
    assert not fails, "\n".join(fails)


def test_every_path_was_reached(aslp, dev):
    """runs last: every row of the two tables ran on the path it names, every path occurs, and the measured ratios"""
    print("\nthe largest err / bar per group:")
    for g, (r, where) in sorted(worst.items()):
        print("    %-24s %.3f   %s" % (g, r, where))
    print("slowest: %s" % ", ".join("%s %.2f s" % kv for kv in sorted(seconds.items(), key=lambda kv: -kv[1])[:4]))
    print("the file so far: %.1f s" % (time.time() - _t0))
    if launch_failed:
        pytest.fail("a launch ended in an error: %s %s" % launch_failed[0])
    assert [n for n in ref.RC_NAMES if "rowconv " + n not in reached] == []
    assert [n for n in ref.FSMN_NAMES if "fsmn " + n not in reached] == []
    rc = [reached["rowconv " + n] for n in ref.RC_NAMES]
    assert {f for f, b in rc} == {0, 4, 8, 16, 21, 32} and {b for f, b in rc} == {0, 4, 8, 16, 21, 32}
    assert {reached["fsmn " + n] for n in ref.FSMN_NAMES} == {(True, True), (True, False), (False, False)}
