"""Xent on CSR targets (aslp_xent_sparse_eval / aslp_xent_sparse_eval_rows) against the dense entry points, bit for bit.

The yardstick is the dense kernel itself: aslp_xent_eval / aslp_softmax_xent_eval are given csr -> dense of the same entries
(xent_sparse_ref.csr_to_dense, a numpy restatement), and the sparse launch must leave the same bits in the diff, in the posteriors and in
the five accumulators -- a target of 0 adds exactly 0 to every sum the kernel forms, so nothing less than equality is due.  Cases: every
case of bn_xent_ref.XENT_CASES that the register-cached kernels serve (all eight per{4,8,16,32}-{scalar,vec} instantiations, both
4100-row cases in which a workgroup takes a second row -- the staging row must have been cleared -- and the misaligned-stride case), each
without and, where the width allows it, with the Softmax, with and without post_out.  Targets: the case's soft matrix with rows overwritten
by the adversarial kinds of xent_sparse_ref (the CPU file checks that each has its property and that every kind is met at every rung).
Inputs' padding is NaN, outputs' padding a sentinel that must survive.  The file takes a few seconds."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import bn_xent_ref as ref
import xent_sparse_ref as sp

pytestmark = pytest.mark.gpu
SENTINEL = ref.SENTINEL
launch_failed = []          # once a launch ended in an error that is no refusal, nothing further is started on the GPU
reached = set()             # (instantiation, softmax)


def guarded(aslp, what, fn):
    if launch_failed:
        pytest.fail("not started: %s ended in an error, and nothing more runs on the GPU behind it\n%s" % launch_failed[0])
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    except AssertionError:
        raise
    except Exception as e:
        launch_failed.append((what, repr(e)))
        raise


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Mat:
    """a [rows x cols] view with leading dimension ld inside a larger buffer: two rows and ld - cols columns of padding, 16 bytes in front"""

    def __init__(self, dev, rows, cols, ld, fill=None, pad=SENTINEL):
        self.ld = ld
        self.buf = torch.full(((rows + 2) * ld + 8,), pad, dtype=torch.float32, device=dev)
        self.v = self.buf[4:4 + (rows + 2) * ld].view(rows + 2, ld)[:rows, :cols]
        if fill is not None:
            self.v.copy_(torch.from_numpy(np.ascontiguousarray(fill, np.float32)).to(dev))
        self.p = C.c_void_p(self.v.data_ptr())
        assert self.v.data_ptr() % 16 == 0

    def padding_intact(self):
        keep = self.v.clone()
        self.v.fill_(SENTINEL)
        ok = bool((self.buf == SENTINEL).all())
        self.v.copy_(keep)
        return ok


def same_bits(a, b):
    return torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int64), b.view(torch.int32 if b.dtype == torch.float32 else torch.int64))


@functools.lru_cache(maxsize=None)
def data(name):
    case = ref.XENT_BY_NAME[name]
    inp = ref.xent_inputs(case)
    return inp, sp.sparse_targets(case, inp)


def test_cases_cover_every_kind_at_every_rung():
    met = sp.coverage()
    for p in sp.RUNGS:
        assert met[p] == sp.wanted_coverage(p)
        dealt = set()
        for c in sp.SPARSE_CASES:
            if sp.rung(c.cols) == p:
                dealt |= set(data(c.name)[1].kinds.values())
        assert dealt == met[p], (p, sorted(met[p] - dealt))


@pytest.mark.parametrize("name", sp.SPARSE_NAMES)
def test_sparse_case(aslp, dev, name):
    inp, t = data(name)
    c = inp.case
    lib, ops, ld = aslp.lib, aslp.ops, c.stride or c.cols + 4
    assert c.kernel == ref.xent_kernel(c.cols, ld % 4 == 0)
    nan = float("nan")
    mat = lambda fill=None, pad=SENTINEL: Mat(dev, c.rows, c.cols, ld, fill, pad)
    y, acts, dense = mat(inp.post, nan), mat(inp.logits, nan), mat(t.dense, nan)
    fw = torch.from_numpy(t.fw).to(dev)
    rb, cols, w = (torch.from_numpy(a).to(dev) for a in (t.row_begin, t.cols, t.weights))
    d = aslp._lib.MatrixDim(c.rows, c.cols, ld)
    stats0 = lambda: torch.from_numpy(ref.STATS0.copy()).to(dev)
    for sm in ((False, True) if ref.softmax_supported(c.cols) else (False,)):
        src = acts if sm else y
        for with_post in (True, False):
            what = "%s%s%s" % (name, " softmax" if sm else "", " +posteriors" if with_post else "")
            # the dense entry point on csr -> dense: the parent's code
            diff_d, post_d, stats_d = mat(), (mat() if with_post else None), stats0()
            if sm:
                fn = lambda: lib.aslp_softmax_xent_eval(src.p, d, dense.p, ld, None, ptr(fw), diff_d.p, ld, ptr(stats_d),
                                                        post_d.p if post_d else None, ld if post_d else 0)
            else:
                fn = lambda: lib.aslp_xent_eval(src.p, d, dense.p, ld, None, ptr(fw), diff_d.p, ld, ptr(stats_d))
            guarded(aslp, what + " dense", fn)
            ops.check_error()
            # the sparse launch with accumulators, twice, and the form that leaves the row statistics
            outs = []
            for k in range(2):
                diff, post, stats = mat(), (mat() if with_post else None), stats0()
                served = guarded(aslp, what, lambda: ops.xent_sparse_eval(src.v, rb, cols, w, fw, diff.v, stats, sm, post.v if post else None))
                ops.check_error()
                assert served == 1, what
                outs.append((diff, post, stats))
            diff_r, post_r, stats_r = mat(), (mat() if with_post else None), stats0()
            rowstats = torch.full((c.rows + 1, 5), SENTINEL, dtype=torch.float64, device=dev)
            served = guarded(aslp, what + " rows",
                             lambda: ops.xent_sparse_eval_rows(src.v, rb, cols, w, fw, diff_r.v, rowstats[:c.rows], sm, post_r.v if post_r else None))
            ops.check_error()
            assert served == 1, what
            guarded(aslp, what + " sum", lambda: ops.xent_sum_rowstats(rowstats[:c.rows], c.rows, 1, stats_r))
            assert bool((rowstats[c.rows] == SENTINEL).all()), (what, "row statistics written past the last row")
            outs.append((diff_r, post_r, stats_r))
            for k, (diff, post, stats) in enumerate(outs):
                where = (what, ("first call", "second call", "rows form")[k])
                assert same_bits(diff.buf, diff_d.buf), (where, "diff", int((diff.v != diff_d.v).sum()))
                assert diff.padding_intact(), (where, "diff's padding")
                if post is not None:
                    if sm:
                        assert same_bits(post.buf, post_d.buf), (where, "posteriors")
                        assert post.padding_intact(), (where, "posteriors' padding")
                    else:
                        assert bool((post.buf == SENTINEL).all()), (where, "posteriors written without the Softmax")
                assert same_bits(stats, stats_d), (where, "statistics", stats.cpu().numpy(), stats_d.cpu().numpy())
            reached.add((c.kernel, sm))


def refused(aslp, dev, rows, cols, softmax, null_row_begin=False, short_stride=False, match="unsupported number of classes"):
    ops = aslp.ops
    ld = cols + 4
    src, diff, post = Mat(dev, rows, cols, ld, np.zeros((rows, cols), np.float32)), Mat(dev, rows, cols, ld), Mat(dev, rows, cols, ld)
    rb = torch.arange(rows + 1, dtype=torch.int32, device=dev)
    tc, tw, fw = torch.zeros(rows, dtype=torch.int32, device=dev), torch.ones(rows, device=dev), torch.ones(rows, device=dev)
    stats = torch.from_numpy(ref.STATS0.copy()).to(dev)
    rowstats = torch.full((rows, 5), SENTINEL, dtype=torch.float64, device=dev)
    inp = src.v
    if short_stride:                        # a view whose rows overlap: cols columns at a stride of cols - 1
        inp = torch.as_strided(src.buf, (rows, cols), (cols - 1, 1), 4)
    for rows_form in (False, True):
        fn = ops.xent_sparse_eval_rows if rows_form else ops.xent_sparse_eval
        served = guarded(aslp, "refusal", lambda: fn(inp, None if null_row_begin else rb, tc, tw, fw, diff.v, rowstats if rows_form else stats,
                                                     softmax, post.v if softmax else None))
        assert served == 0
        with pytest.raises(RuntimeError, match=match):
            ops.check_error()
    torch.cuda.synchronize()
    assert bool((diff.buf == SENTINEL).all()) and bool((post.buf == SENTINEL).all()) and bool((rowstats == SENTINEL).all())
    assert np.array_equal(stats.cpu().numpy(), ref.STATS0)


@pytest.mark.parametrize("cols", [8193, 20000])
def test_refuses_wider_rows(aslp, dev, cols):
    assert aslp.lib.aslp_xent_sparse_supported(cols, 0) == 0 and aslp.lib.aslp_xent_sparse_supported(8192, 0) == 1
    refused(aslp, dev, 4, cols, False)


def test_refuses_softmax_at_512(aslp, dev):
    assert aslp.lib.aslp_xent_sparse_supported(512, 1) == 0 and aslp.lib.aslp_xent_sparse_supported(513, 1) == 1
    assert aslp.lib.aslp_xent_sparse_supported(512, 0) == 1 and aslp.lib.aslp_xent_sparse_supported(0, 0) == 0
    refused(aslp, dev, 4, 512, True)


def test_refuses_null_row_begin(aslp, dev):
    refused(aslp, dev, 4, 600, False, null_row_begin=True, match="null argument")


def test_refuses_stride_below_cols(aslp, dev):
    refused(aslp, dev, 4, 600, False, short_stride=True, match="no stride smaller than the number of columns")


def test_every_instantiation_was_reached(aslp, dev):
    """runs last"""
    if launch_failed:
        pytest.fail("a launch ended in an error: %s %s" % launch_failed[0])
    want = {("per%d-%s" % (p, m), sm) for p in sp.RUNGS for m in ("scalar", "vec") for sm in (False, True)}
    assert sorted(want - reached) == []
