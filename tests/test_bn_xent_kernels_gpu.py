"""The BatchNormalization and Xent kernels of csrc/nn_fused.hip, every instantiation the host can pick, against the float64 models of
tests/bn_xent_ref.py (pinned to the oracle by tests/test_bn_xent_ref_cpu.py): the three-launch path (one column per access, 16-byte accesses,
and a panel shape whose rows start 4 bytes off), bn_forward_panel / bn_backward_panel at 4, 8 and 16 slots and at both ends of each,
bn_forward_coop / bn_backward_coop at Q = 4, 3 and 2 workgroups per panel with 4, 8 and 16 slots and an uneven last chunk, each backward
with and without the folded Sigmoid, with and without a stored xhat, with and without the folded step, once without in_diff, the
per-workgroup maxima, aslp_bn_forward_stats at every Q its host rule picks; xent_rows_kernel at 4 / 8 / 16 / 32 slots in both column maps,
with posteriors and with activations in, label, one-hot and soft targets, the streaming kernel, the second row of a workgroup, labels
outside [0, cols); and what the entry points refuse.  Which BatchNormalization kernel serves a shape depends on the device's CU count: every
case asks aslp_bn_path and asserts the instantiation bn_xent_ref.BN_CASES names (for 256 CUs).

Every case makes two consecutive calls that carry the component's state; buffers are padded and the padding is poisoned (inputs: NaN;
outputs: SENTINEL, which must still be there afterwards).

The bar comes from the oracle, never from the GPU: per case and output the GPU's distance to float64 (relative l2; largest element as
oracle_lib.max_err measures it, evaluated on the device in float64) may be MARGIN x the oracle's distance on the same output, with floors
where fp32 is simply accurate (bn_xent_ref.FLOOR_*).  A BatchNormalization matrix is held to that bar twice: over all its columns, and
over the ordinary columns alone (bn_xent_ref.BN_GROUPS: over all columns the oracle's own 7.5e-4 on the column of one value would let
1e-4 through everywhere else); the batch mean and inv_std are also held to four half-ulps element by element.  The double accumulators
keep 1e-12 rows + 1e-9, the five Xent sums rtol 1e-5 / atol 1e-6 with `frames` and `correct` exact, and where the oracle is within 1e-5
of float64 the project's 1e-4 is asserted against the oracle directly.

MEASURED on an MI355X (256 CUs, no case skipped): the worst margin any output needs -- its distance over the oracle's, counted where it lies
above the floor -- per group, as test_every_instantiation_was_reached prints it:
    bn-forward       1.29   (panel-2x16, act; ordinary columns alone: within the floors)
    bn-backward      1.87   (coop-1024x2752, in_diff; ordinary columns alone 1.54, panel-256x16, D)
    bn-step          2.10   (coop-512x64, in_diff of the second call: 1.7e-7 against the oracle's 8.2e-8, 1.4 floors; ordinary columns 1.18)
    bn-stats         1.00   (stats-1000x2048, act)
    xent-posteriors  0      every diff within the floors (by distance alone 0.81 of the oracle's at the worst, 8x1028-ld1029 soft)
    xent-softmax     0      every diff and every posterior within the floors (0.50)
MARGIN = 3 is the smallest of 2, 3, 4 that is >= 1.3 x 2.10; no ratio is above 3.  On the column at mean 100 the one-pass double variance
lies where float64 lies (inv_std within four half-ulps on every case) -- once it divides by rows in double: before that the kernels
multiplied by the fp32 1 / rows, and this file found inv_std off on that column wherever rows is no power of two (three-100x37: 1.1e-4,
three-7x5: 2.7e-4 and 4.7e-4; 24 of the 61 tests failed), and 0.32 relative l2 / 0.45 off on the column of one value (three-100x37: a
"variance" of 6e-7 where it is 0).
A batch of one row (panel-1x16) came back with in_diff up to 4.9e-4 where the reference has exactly 0; the host now zeroes it.
The file takes 7.8 s on the MI355X, 5.7 s of it in the cases; the slowest test is coop-1024x2752 at 1.0 s.
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import bn_xent_ref as ref
from test_bn_xent_ref_cpu import bn_distances, bn_oracle_sequence, xent_data

pytestmark = pytest.mark.gpu
SENTINEL = ref.SENTINEL
REFUSALS = ("xhat == NULL is only served", "unsupported number of classes", "no room for the per-row statistics", "statistics layout does not match")
_t0 = time.time()
launch_failed = []          # [(what, error)]: once a launch ended in an error, nothing further is started on the GPU
reached = {}                # case -> what aslp_bn_path / the Xent host rule picked
worst = {}                  # (test group, column group) -> (ratio, where)
seconds = {}                # test -> seconds


def on_gpu(aslp, what, fn):
    """fn() behind the guard, followed by the library's error check and a synchronize: an error other than a refused argument stops every
    later GPU call of this file"""
    if launch_failed:
        pytest.fail("not started: %s ended in an error, and nothing more runs on the GPU behind it\n%s" % launch_failed[0])
    try:
        out = fn()
        aslp.ops.check_error()
        torch.cuda.synchronize()
        aslp.ops.check_error()
        return out
    except RuntimeError as e:
        if not any(r in str(e) for r in REFUSALS):
            launch_failed.append((what, repr(e)))
        raise
    except AssertionError:
        raise
    except Exception as e:
        launch_failed.append((what, repr(e)))
        raise


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def f32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


class Mat:
    """a [rows x cols] view with leading dimension ld inside a larger buffer: two rows and ld - cols columns of padding, 16 bytes in front;
    offset: the view starts 4 bytes off a 16-byte boundary"""

    def __init__(self, dev, rows, cols, fill=None, pad=SENTINEL, ld=None, offset=False):
        self.ld = ld or cols + 4
        start = 4 + (1 if offset else 0)
        self.buf = torch.full(((rows + 2) * self.ld + 8,), pad, dtype=torch.float32, device=dev)
        self.v = self.buf[start:start + (rows + 2) * self.ld].view(rows + 2, self.ld)[:rows, :cols]
        if fill is not None:
            self.v.copy_(f32(fill, dev))
        self.p = C.c_void_p(self.v.data_ptr())
        assert (self.v.data_ptr() % 16 == 4) == bool(offset)

    def padding_intact(self):
        keep = self.v.clone()
        self.v.fill_(SENTINEL)
        ok = bool((self.buf == SENTINEL).all())
        self.v.copy_(keep)
        return ok


def P(m):
    return m.p if m is not None else None


def L(m):
    return m.ld if m is not None else 0


def gdist(t, want, dev, groups=True):
    """distances of a device tensor to a float64 host array, formed on the device: per column group (bn_xent_ref.group_dist), or
    (relative l2, oracle_lib.max_err) over everything"""
    r = torch.from_numpy(np.atleast_2d(np.asarray(want, np.float64))).to(dev)
    a = t.double().reshape(r.shape) if t.dim() == 1 else t.double()
    d = a - r
    if groups:
        e2, r2, em, rm = torch.stack([(d * d).sum(0), (r * r).sum(0), d.abs().amax(0), r.abs().amax(0)]).cpu().numpy()
        return ref.group_dist(e2, r2, em, rm, r.shape[0])
    num, den, em, rm = torch.stack([d.norm(), r.norm(), d.abs().max(), r.abs().max()]).cpu().numpy()
    return float(num / den if den > 0 else num), float(em / max(1.0, rm))


def judge(test_group, where, d, d_orc, fails, colgroup="all"):
    """one output against its bar; -> the GPU / oracle ratio"""
    b, r = ref.bar(d_orc), ref.ratio(d, d_orc)
    if not r <= worst.get((test_group, colgroup), (0.0, ""))[0]:
        worst[(test_group, colgroup)] = (r, where)
    if not (d[0] <= b[0] and d[1] <= b[1]):
        fails.append("%s %s [%s]: GPU %.3e / %.3e, oracle %.3e / %.3e, bar %.3e / %.3e, ratio %.2f" % ((test_group, where, colgroup) + d + d_orc + b + (r,)))
    return r


def compare_bn(test_group, where, key, t, want, orc, d_orc, dev, fails):
    """an output against MARGIN x the oracle's distance: over all columns, and a matrix also over the ordinary columns alone (not at one or
    two rows, where in_diff cancels to zero and a relative distance says nothing); the batch mean and inv_std element by element"""
    d = gdist(t, want, dev)
    rows = t.shape[0] if t.dim() == 2 else 0
    judged = ("all", "rest") if rows > 2 else ("all",)
    rs = [judge(test_group, "%s %s" % (where, key), d[g], d_orc[g], fails, g) for g in judged]
    if key in ("mean", "inv_std"):
        # the mean is fl(fl(sum) fl(1 / rows)) of a sum exact in double, inv_std 1 / sqrt(fl(var) + floor) of a variance exact to double
        # rounding: three half-ulps each, whatever the column -- the oracle's fp32 sums are a bar only where they happen to be lucky
        w = np.asarray(want, np.float64)
        e = np.abs(t.double().cpu().numpy() - w) / np.where(w != 0, np.abs(w), 1.0)
        if not e.max() <= ref.FLOOR_EL:
            fails.append("%s %s %s: column %d is %.3e relative from float64" % (test_group, where, key, int(e.argmax()), e.max()))
    close = [g for g in judged if d_orc[g][0] <= 1e-5]
    if close:   # the project's tolerance, against the oracle itself
        do = gdist(t, orc, dev)
        for g in close:
            if not do[g][0] < 1e-4:
                fails.append("%s %s %s [%s]: %.3e from the oracle" % (test_group, where, key, g, do[g][0]))
    return "%s %.2f" % (key, max(rs))


def compare_acc(where, key, t, want, rows, fails):
    e = ref.rel_l2(t.cpu().numpy(), want)
    if not e < 1e-12 * rows + 1e-9:
        fails.append("%s %s: %.3e from float64" % (where, key, e))


def bn_path(aslp, case):
    """what the library picks for this shape on this device, against what the table names; a cooperative case that lands elsewhere on a
    device with another CU count is skipped"""
    q, slots = C.c_int(-1), C.c_int(-1)
    path = aslp.lib.aslp_bn_path(case.rows, case.cols, C.byref(q), C.byref(slots))
    got = (("three", "panel", "coop")[path], q.value, slots.value)
    want = ("panel", 1, 4) if case.offset else (case.path, case.q, case.slots)   # (the query speaks of aligned operands)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if got != want and case.path == "coop" and cus != 256:
        pytest.skip("%s is served by %s on this device's %d CUs, not by the cooperative kernel the table names for 256" % (case.name, got, cus))
    assert got == want, (case.name, got, want, cus)
    return got


class BnState:
    def __init__(self, inp, dev):
        cols = inp.case.cols
        self.scale, self.shift, self.dscale, self.dshift = (f32(a, dev) for a in (inp.scale, inp.shift, inp.dscale0, inp.dshift0))
        self.mean, self.inv = torch.full((cols,), SENTINEL, device=dev), torch.full((cols,), SENTINEL, device=dev)
        self.accm, self.accv = torch.zeros(cols, dtype=torch.float64, device=dev), torch.zeros(cols, dtype=torch.float64, device=dev)


def bn_forward(aslp, dev, inp, st, k, want_out, want_xhat, want_act, what):
    c = inp.case
    x = Mat(dev, c.rows, c.cols, inp.x[k], float("nan"), offset=c.offset)
    out, xhat, act = (Mat(dev, c.rows, c.cols, offset=c.offset) if w else None for w in (want_out, want_xhat, want_act))
    d = aslp._lib.MatrixDim(c.rows, c.cols, x.ld)
    on_gpu(aslp, what, lambda: aslp.lib.aslp_bn_forward_act(x.p, d, P(out), L(out), P(xhat), L(xhat), ptr(st.scale), ptr(st.shift), ptr(st.mean), ptr(st.inv),
                                                            ptr(st.accm), ptr(st.accv), 1e-7, P(act), L(act)))
    return x, d, out, xhat, act


def bn_backward(aslp, dev, inp, st, k, x, d, xhat, act, has_y, step, what, with_in_diff=True, po=None):
    c = inp.case
    od = Mat(dev, c.rows, c.cols, inp.od[k], float("nan"), offset=c.offset)
    ind = Mat(dev, c.rows, c.cols, offset=c.offset)
    y = act if has_y else None
    pi, li = (ind.p, ind.ld) if with_in_diff else (None, 0)
    lib = aslp.lib
    if po is not None:
        fn = lambda: lib.aslp_bn_backward_step_p(d, od.p, od.ld, P(xhat), L(xhat), ptr(st.scale), ptr(st.shift), ptr(st.inv), ptr(st.dscale), ptr(st.dshift),
                                                 ref.MMT, ref.LR, pi, li, P(y), L(y), x.p, ptr(st.mean), C.byref(po))
    elif step:
        fn = lambda: lib.aslp_bn_backward_step(d, od.p, od.ld, P(xhat), L(xhat), ptr(st.scale), ptr(st.shift), ptr(st.inv), ptr(st.dscale), ptr(st.dshift),
                                               ref.MMT, ref.LR, pi, li, P(y), L(y), x.p, ptr(st.mean))
    else:
        fn = lambda: lib.aslp_bn_backward_act(x.p, d, od.p, od.ld, P(xhat), L(xhat), ptr(st.scale), ptr(st.mean), ptr(st.inv), ptr(st.dscale), ptr(st.dshift),
                                              ref.MMT, pi, li, P(y), L(y))
    on_gpu(aslp, what, fn)
    return ind


def run_sequence(aslp, dev, inp, has_y, step, rc, want, orc, d_orc, fails):
    """two consecutive forward + backward calls on the GPU, every output against its bar.  Forward forms: out + xhat (no Sigmoid), out + xhat
    + act (Sigmoid, xhat stored), act alone (Sigmoid, xhat recomputed), out alone (no Sigmoid, xhat recomputed)"""
    c = inp.case
    st = BnState(inp, dev)
    bgroup = "bn-step" if step else "bn-backward"
    for k in range(2):
        what = "%s y%d step%d recompute%d call%d" % (c.name, has_y, step, rc, k)
        x, d, out, xhat, act = bn_forward(aslp, dev, inp, st, k, not (has_y and rc), not rc, has_y, what + " forward")
        line = []
        for key, m in (("out", out), ("xhat", xhat), ("act", act)):
            if m is not None:
                line.append(compare_bn("bn-forward", what, key, m.v, want[k][key], orc[k][key], d_orc[k][key], dev, fails))
                assert m.padding_intact(), (what, key, "padding")
        for key, t in (("mean", st.mean), ("inv_std", st.inv)):
            line.append(compare_bn("bn-forward", what, key, t, want[k][key], orc[k][key], d_orc[k][key], dev, fails))
        compare_acc(what, "acc_means", st.accm, want[k]["acc_means"], c.rows, fails)
        compare_acc(what, "acc_vars", st.accv, want[k]["acc_vars"], c.rows, fails)
        before = st.scale.clone(), st.shift.clone()
        ind = bn_backward(aslp, dev, inp, st, k, x, d, xhat, act, has_y, step, what + " backward")
        for key, t in (("in_diff", ind.v), ("D", xhat.v if xhat is not None else None), ("dscale", st.dscale), ("dshift", st.dshift), ("scale", st.scale), ("shift", st.shift)):
            if t is not None and (step or key not in ("scale", "shift")):
                line.append(compare_bn(bgroup, what, key, t, want[k][key], orc[k][key], d_orc[k][key], dev, fails))
        if not step:
            assert torch.equal(before[0], st.scale) and torch.equal(before[1], st.shift), (what, "scale / shift without a step")
        assert ind.padding_intact() and (xhat is None or xhat.padding_intact()), (what, "padding behind the backward")
        print("%-52s %s" % (what, "  ".join(line)))


@pytest.mark.parametrize("name", ref.BN_NAMES)
def test_bn_case(aslp, oracle, dev, name):
    t0 = time.time()
    case = ref.BN_BY_NAME[name]
    got = bn_path(aslp, case)
    inp = ref.bn_inputs(case)
    fails, cache = [], {}
    for has_y in (False, True):
        for step in (False, True):
            want = ref.bn_sequence(inp, has_y, step, cache)
            orc = bn_oracle_sequence(oracle, inp, has_y, step)
            d_orc = bn_distances(oracle, orc, want)
            for rc in ((False, True) if case.path != "three" else (False,)):
                run_sequence(aslp, dev, inp, has_y, step, rc, want, orc, d_orc, fails)
            if has_y and step:   # once without in_diff: only the gradients and the step may change
                st = BnState(inp, dev)
                what = "%s no in_diff" % name
                x, d, out, xhat, act = bn_forward(aslp, dev, inp, st, 0, True, True, True, what + " forward")
                kept = xhat.buf.clone()
                ind = bn_backward(aslp, dev, inp, st, 0, x, d, xhat, act, True, True, what + " backward", with_in_diff=False)
                assert torch.equal(kept, xhat.buf) and bool((ind.buf == SENTINEL).all()), (what, "xhat or in_diff written")
                for key, t in (("dscale", st.dscale), ("dshift", st.dshift), ("scale", st.scale), ("shift", st.shift)):
                    compare_bn("bn-step", what, key, t, want[0][key], orc[0][key], d_orc[0][key], dev, fails)
            if has_y and not step and case.path == "three":
                # act alone on the three-launch path; and no backward without a stored xhat there: an error, nothing launched
                st = BnState(inp, dev)
                what = "%s act alone" % name
                x, d, out, xhat, act = bn_forward(aslp, dev, inp, st, 0, False, False, True, what + " forward")
                for key, t in (("act", act.v), ("mean", st.mean), ("inv_std", st.inv)):
                    compare_bn("bn-forward", what, key, t, want[0][key], orc[0][key], d_orc[0][key], dev, fails)
                assert act.padding_intact()
                keep = st.dscale.clone(), st.dshift.clone()
                with pytest.raises(RuntimeError, match="xhat == NULL is only served"):
                    ind = bn_backward(aslp, dev, inp, st, 0, x, d, None, act, True, False, what + " refused backward")
                torch.cuda.synchronize()
                assert torch.equal(keep[0], st.dscale) and torch.equal(keep[1], st.dshift)
    reached[name] = got
    seconds["bn " + name] = time.time() - t0
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", [c.name for c in ref.BN_CASES if c.path == "coop"])
def test_bn_coop_leaves_every_workgroups_maximum(aslp, dev, name):
    """aslp_bn_backward_step_p on a device that is shared (no launch may wait for all its workgroups): the parts are left, one per workgroup
    b = q P + p, each max |in_diff| over rows q rp .. min(rows, (q + 1) rp), columns 32 p .. 32 p + 31, bit for bit"""
    case = ref.BN_BY_NAME[name]
    _, Q, _ = bn_path(aslp, case)
    inp = ref.bn_inputs(case)
    Pn, rp = case.cols // ref.COOP_COLS, -(-case.rows // Q)
    st = BnState(inp, dev)
    x, d, out, xhat, act = bn_forward(aslp, dev, inp, st, 0, False, False, True, name + " forward")
    parts = torch.full((Pn * Q + 8,), SENTINEL, device=dev)
    po = aslp._lib.PlanesOut()
    po.parts = parts.data_ptr()
    aslp.lib.aslp_device_shared(1)
    try:
        ind = bn_backward(aslp, dev, inp, st, 0, x, d, None, act, True, True, name + " backward with parts", po=po)
    finally:
        aslp.lib.aslp_device_shared(0)
    assert po.planes_written == 0 and po.nparts == Pn * Q
    want = torch.cat([ind.v[q * rp:min(case.rows, (q + 1) * rp)].abs().reshape(-1, Pn, ref.COOP_COLS).amax((0, 2)) for q in range(Q)])
    assert torch.equal(parts[:Pn * Q], want), (parts[:Pn * Q] != want).nonzero().flatten().tolist()[:8]
    assert bool((parts[Pn * Q:] == SENTINEL).all()) and ind.padding_intact()


@pytest.mark.parametrize("rows,cols", ref.BN_STATS_SHAPES)
def test_bn_forward_from_column_partials(aslp, oracle, dev, rows, cols):
    """aslp_bn_forward_stats with partials formed here in float64 per 32-row group (sum x, sum fl32(x x), sum x x), so that the case does not
    depend on the product kernels; two calls, the second adds to the running sums"""
    t0 = time.time()
    case = ref.BnCase("stats-%dx%d" % (rows, cols), rows, cols, "stats", ref.bn_stats_q(rows, cols), 0, False)
    inp = ref.bn_inputs(case, seed=3000 + rows + cols)
    want = ref.bn_sequence(inp, True, False)
    orc = bn_oracle_sequence(oracle, inp, True, False)
    d_orc = bn_distances(oracle, orc, want)
    st = BnState(inp, dev)
    groups, ld, fails = (rows + 31) // 32, cols + 4, []
    for k in range(2):
        x = Mat(dev, rows, cols, inp.x[k], float("nan"))
        xp = torch.zeros(groups * 32, cols, device=dev)
        xp[:rows] = x.v
        stats = torch.full((3, groups, ld), float("nan"), dtype=torch.float64, device=dev)
        stats[0, :, :cols] = xp.double().view(groups, 32, cols).sum(1)
        stats[1, :, :cols] = (xp * xp).double().view(groups, 32, cols).sum(1)
        stats[2, :, :cols] = (xp.double() * xp.double()).view(groups, 32, cols).sum(1)
        out, act = Mat(dev, rows, cols), Mat(dev, rows, cols)
        d = aslp._lib.MatrixDim(rows, cols, x.ld)
        what = "%s call%d" % (case.name, k)
        ran = on_gpu(aslp, what, lambda: aslp.lib.aslp_bn_forward_stats(x.p, d, out.p, out.ld, ptr(st.scale), ptr(st.shift), ptr(st.mean), ptr(st.inv), ptr(st.accm),
                                                                        ptr(st.accv), 1e-7, act.p, act.ld, ptr(stats), groups, ld))
        assert ran == 1, what
        line = [compare_bn("bn-stats", what, key, t, want[k][key], orc[k][key], d_orc[k][key], dev, fails)
                for key, t in (("out", out.v), ("act", act.v), ("mean", st.mean), ("inv_std", st.inv))]
        compare_acc(what, "acc_means", st.accm, want[k]["acc_means"], rows, fails)
        compare_acc(what, "acc_vars", st.accv, want[k]["acc_vars"], rows, fails)
        assert out.padding_intact() and act.padding_intact()
        print("%-52s Q %d  %s" % (what, case.q, "  ".join(line)))
        if k == 1:   # a `groups` that does not match: an error, 0, nothing written
            out2 = Mat(dev, rows, cols)
            keep = st.accm.clone()
            with pytest.raises(RuntimeError, match="statistics layout does not match"):
                on_gpu(aslp, what, lambda: aslp.lib.aslp_bn_forward_stats(x.p, d, out2.p, out2.ld, ptr(st.scale), ptr(st.shift), ptr(st.mean), ptr(st.inv), ptr(st.accm),
                                                                          ptr(st.accv), 1e-7, None, 0, ptr(stats), groups + 1, ld))
            torch.cuda.synchronize()
            assert bool((out2.buf == SENTINEL).all()) and torch.equal(keep, st.accm)
    reached[case.name] = ("stats", case.q, 0)
    seconds["bn " + case.name] = time.time() - t0
    assert not fails, "\n".join(fails)


def test_bn_forward_from_column_partials_declines_other_widths(aslp, dev):
    """(100, 48): cols % 32 != 0 -- 0, no error, nothing written"""
    rows, cols = 100, 48
    x, out = Mat(dev, rows, cols, np.ones((rows, cols), np.float32)), Mat(dev, rows, cols)
    vec = [torch.full((cols,), SENTINEL, device=dev) for _ in range(4)]
    acc = [torch.zeros(cols, dtype=torch.float64, device=dev) for _ in range(2)]
    stats = torch.zeros(3, 4, cols, dtype=torch.float64, device=dev)
    d = aslp._lib.MatrixDim(rows, cols, x.ld)
    ran = on_gpu(aslp, "stats 100x48", lambda: aslp.lib.aslp_bn_forward_stats(x.p, d, out.p, out.ld, ptr(vec[0]), ptr(vec[1]), ptr(vec[2]), ptr(vec[3]), ptr(acc[0]), ptr(acc[1]),
                                                                             1e-7, None, 0, ptr(stats), 4, cols))
    assert ran == 0 and bool((out.buf == SENTINEL).all()) and all(bool((v == SENTINEL).all()) for v in vec) and not acc[0].any() and not acc[1].any()


# ---- Xent -----------------------------------------------------------------------------------------------------------------------------
def check_xent(group, what, inp, r, diff, post, stats, dev, fails):
    d = gdist(diff.v, r["diff"], dev, groups=False)
    rs = [judge(group, what + " diff", d, r["d_diff"], fails)]
    do = gdist(diff.v, r["orc_diff"], dev, groups=False)   # (the oracle lies within 1e-5 of float64 on every case: test_bn_xent_ref_cpu)
    if not do[0] < 1e-4:
        fails.append("%s %s diff: %.3e from the oracle" % (group, what, do[0]))
    if post is not None:
        rs.append(judge(group, what + " posteriors", gdist(post.v, r["post"], dev, groups=False), r["d_post"], fails))
        assert post.padding_intact(), (what, "posteriors' padding")
    assert diff.padding_intact(), (what, "diff's padding")
    got = stats.cpu().numpy() - ref.STATS0
    if not (got[0] == r["sums"][0] and got[1] == r["sums"][1] and np.allclose(got, r["sums"], rtol=1e-5, atol=1e-6)):
        fails.append("%s %s sums: %s, float64 %s" % (group, what, got, r["sums"]))
    return "%s %s" % (what.split(" ", 1)[1], "/".join("%.2f" % v for v in rs))


@pytest.mark.parametrize("name", ref.XENT_NAMES)
def test_xent_case(aslp, oracle, dev, name):
    t0 = time.time()
    inp, res = xent_data(oracle, name)
    c = inp.case
    lib, ld = aslp.lib, c.stride or c.cols + 4
    assert c.kernel == ref.xent_kernel(c.cols, ld % 4 == 0)
    mat = lambda fill=None, pad=SENTINEL: Mat(dev, c.rows, c.cols, fill, pad, ld=ld)
    nan = float("nan")
    y, acts, onehot, soft = mat(inp.post, nan), mat(inp.logits, nan), mat(inp.onehot, nan), mat(inp.soft, nan)
    labels, fw = torch.from_numpy(inp.labels).to(dev), f32(inp.fw, dev)
    d = aslp._lib.MatrixDim(c.rows, c.cols, ld)
    fails, line = [], []
    for sm in ((False, True) if ref.softmax_supported(c.cols) else (False,)):
        group, src = ("xent-softmax", acts) if sm else ("xent-posteriors", y)
        for target in ref.TARGETS:
            r = res[("soft" if target == "soft" else "onehot", sm)]
            t = soft if target == "soft" else onehot
            for with_post in ((True, False) if sm and target != "labels" else (False,)):
                what = "%s %s%s%s" % (name, target, " softmax" if sm else "", " +posteriors" if with_post else "")
                diff, post = mat(), (mat() if with_post else None)
                stats = torch.from_numpy(ref.STATS0.copy()).to(dev)
                if target == "labels":
                    fn = lambda: lib.aslp_xent_eval_p(src.p, d, ptr(labels), ptr(fw), diff.p, ld, ptr(stats), int(sm), None)
                elif sm:
                    fn = lambda: lib.aslp_softmax_xent_eval(src.p, d, t.p, ld, None, ptr(fw), diff.p, ld, ptr(stats), P(post), L(post))
                else:
                    fn = lambda: lib.aslp_xent_eval(src.p, d, t.p, ld, None, ptr(fw), diff.p, ld, ptr(stats))
                on_gpu(aslp, what, fn)
                line.append(check_xent(group, what, inp, r, diff, post, stats, dev, fails))
    print("xent %-14s %-13s %s" % (name, c.kernel, "  ".join(line)))
    reached["xent " + name] = c.kernel
    seconds["xent " + name] = time.time() - t0
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("cols", [512, 8193])
def test_softmax_xent_refuses_other_widths(aslp, dev, cols):
    rows = 4
    acts, diff, post = Mat(dev, rows, cols, np.zeros((rows, cols), np.float32)), Mat(dev, rows, cols), Mat(dev, rows, cols)
    labels, fw = torch.zeros(rows, dtype=torch.int32, device=dev), torch.ones(rows, device=dev)
    stats = torch.from_numpy(ref.STATS0.copy()).to(dev)
    d = aslp._lib.MatrixDim(rows, cols, acts.ld)
    lib = aslp.lib
    for fn in (lambda: lib.aslp_softmax_xent_eval(acts.p, d, None, 0, ptr(labels), ptr(fw), diff.p, diff.ld, ptr(stats), post.p, post.ld),
               lambda: lib.aslp_xent_eval_p(acts.p, d, ptr(labels), ptr(fw), diff.p, diff.ld, ptr(stats), 1, None)):
        with pytest.raises(RuntimeError, match="unsupported number of classes"):
            on_gpu(aslp, "softmax xent at %d classes" % cols, fn)
        torch.cuda.synchronize()
        assert bool((diff.buf == SENTINEL).all()) and bool((post.buf == SENTINEL).all()) and np.array_equal(stats.cpu().numpy(), ref.STATS0)


def test_xent_rows_refuses_without_room(aslp, dev):
    rows, cols = 4, 600
    acts, diff = Mat(dev, rows, cols, np.zeros((rows, cols), np.float32)), Mat(dev, rows, cols)
    labels, fw = torch.zeros(rows, dtype=torch.int32, device=dev), torch.ones(rows, device=dev)
    d = aslp._lib.MatrixDim(rows, cols, acts.ld)
    with pytest.raises(RuntimeError, match="no room for the per-row statistics"):
        on_gpu(aslp, "xent rows without room", lambda: aslp.lib.aslp_xent_eval_rows(acts.p, d, ptr(labels), ptr(fw), diff.p, diff.ld, None, 1, None))
    torch.cuda.synchronize()
    assert bool((diff.buf == SENTINEL).all())


def test_every_instantiation_was_reached(aslp, dev):
    """runs last: every row of the two tables was reached (none skipped on 256 CUs), and the measured ratios"""
    print("\nthe worst margin an output needs (bn_xent_ref.ratio), per group and column group:")
    for g in ("bn-forward", "bn-backward", "bn-step", "bn-stats", "xent-posteriors", "xent-softmax"):
        worst.setdefault((g, "all"), (0.0, "every output within the floors"))
    for (g, cg), (r, where) in sorted(worst.items()):
        print("    %-16s %-8s %.2f   %s" % (g, cg, r, where))
    print("slowest: %s" % ", ".join("%s %.1f s" % kv for kv in sorted(seconds.items(), key=lambda kv: -kv[1])[:4]))
    print("the file so far: %.1f s" % (time.time() - _t0))
    if launch_failed:
        pytest.fail("a launch ended in an error: %s %s" % launch_failed[0])
    if torch.cuda.get_device_properties(0).multi_processor_count == 256:
        assert [n for n in ref.BN_NAMES if n not in reached] == []
    assert [n for n in ref.BN_NAMES if n in reached and ref.BN_BY_NAME[n].path != "coop" and reached[n][0] == "coop"] == []
    assert [n for n in ref.XENT_NAMES if "xent " + n not in reached] == []
    assert ["stats-%dx%d" % s for s in ref.BN_STATS_SHAPES if "stats-%dx%d" % s not in reached] == []
