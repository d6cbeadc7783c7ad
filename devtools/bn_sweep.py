#!/usr/bin/env python3
"""The BatchNormalization kernels (csrc/nn_fused.hip) on the cases of their test -> one line per call: what aslp_bn_path answers for the shape
and a hash of every buffer the call may write, padding included.  Two builds that compute the same bits write identical files:

    timeout 600 python devtools/bn_sweep.py OUT.txt            (on each build, on the same machine: the path depends on the CU count)
    cmp OLD.txt NEW.txt

Shapes, seeds, buffers and the launches are those of tests/test_bn_xent_kernels_gpu.py (bn_xent_ref.BN_CASES, BN_STATS_SHAPES, bn_inputs; Mat,
BnState, bn_forward, bn_backward); nothing is restated here but the float64 column partials aslp_bn_forward_stats reads, which that file forms
inside its test.  Per case: two consecutive calls (they carry the component's state) of forward + backward for every Sigmoid folded or not x
xhat stored or recomputed (where the path allows) x step or not, once without in_diff; on the cooperative cases once with the workgroups'
maxima left; the planes from the launch at the shapes of test_kernels_gpu.test_bn_backward_leaves_in_diff_planes; aslp_bn_forward_stats at
its five shapes with and without activation planes.  on_gpu raises at the first launch that reports an error, which ends the sweep."""
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
PLANES_SHAPES = [(1024, 2048, True), (1024, 2048, False), (1000, 1024, True), (256, 2048, True)]   # test_bn_backward_leaves_in_diff_planes


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else "bn_sweep.txt"
    import torch
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import aslp_import
    import bn_xent_ref as ref
    import test_bn_xent_kernels_gpu as t
    aslp = aslp_import.load()
    aslp.ops.use_torch_stream()
    dev = torch.device("cuda:0")
    lib, vp, i32 = aslp.lib, C.c_void_p, C.c_int
    lib.aslp_bn_forward_stats_p.restype = i32
    lib.aslp_bn_forward_stats_p.argtypes = [vp, aslp._lib.MatrixDim, vp, i32, vp, vp, vp, vp, vp, vp, C.c_float, vp, i32, vp, i32, i32, C.POINTER(aslp._lib.PlanesOut)]

    def sha(*bufs):
        torch.cuda.synchronize()
        return " ".join("-" if b is None else hashlib.sha1((b.buf if isinstance(b, t.Mat) else b).cpu().numpy().tobytes()).hexdigest()[:16] for b in bufs)

    def bn_path(rows, cols):
        q, slots = i32(-1), i32(-1)
        return "path %d q %d slots %d" % (lib.aslp_bn_path(rows, cols, C.byref(q), C.byref(slots)), q.value, slots.value)

    def state(st):
        return sha(st.mean, st.inv, st.accm, st.accv, st.dscale, st.dshift, st.scale, st.shift)

    class Planes:
        """two fp16 planes and their bound word for a PlanesOut, poisoned"""

        def __init__(self, rows, cols, bound=0):
            self.ld = cols + 4
            self.hi, self.lo = (torch.full((rows + 2, self.ld), 7.0, dtype=torch.float16, device=dev) for _ in range(2))
            self.slot = torch.full((4,), bound, dtype=torch.int32, device=dev)
            self.po = aslp._lib.PlanesOut()
            self.po.hi, self.po.lo, self.po.ld, self.po.slot = self.hi.data_ptr(), self.lo.data_ptr(), self.ld, self.slot.data_ptr()

    with open(path, "w") as out:
        def line(what, rows, cols, *hashes):
            out.write("%s -> %s | %s\n" % (what, bn_path(rows, cols), " | ".join(hashes)))
            out.flush()

        for case in ref.BN_CASES:
            inp = ref.bn_inputs(case)
            rcs = (False, True) if lib.aslp_bn_path(case.rows, case.cols, None, None) != 0 and not case.offset else (False,)
            for has_y in (False, True):
                for rc in rcs:
                    for step in (False, True):
                        st = t.BnState(inp, dev)
                        for k in range(2):
                            what = "%s y%d recompute%d step%d call%d" % (case.name, has_y, rc, step, k)
                            x, d, o, xhat, act = t.bn_forward(aslp, dev, inp, st, k, not (has_y and rc), not rc, has_y, what + " forward")
                            line(what + " forward", case.rows, case.cols, sha(o, xhat, act), state(st))
                            ind = t.bn_backward(aslp, dev, inp, st, k, x, d, xhat, act, has_y, step, what + " backward")
                            line(what + " backward", case.rows, case.cols, sha(xhat, ind), state(st))
            st = t.BnState(inp, dev)
            what = "%s no in_diff" % case.name
            x, d, o, xhat, act = t.bn_forward(aslp, dev, inp, st, 0, True, True, True, what + " forward")
            ind = t.bn_backward(aslp, dev, inp, st, 0, x, d, xhat, act, True, True, what + " backward", with_in_diff=False)
            line(what, case.rows, case.cols, sha(o, xhat, act, ind), state(st))
            if case.path == "coop":   # the workgroups' maxima, as test_bn_coop_leaves_every_workgroups_maximum asks for them
                st = t.BnState(inp, dev)
                what = "%s max_parts" % case.name
                x, d, o, xhat, act = t.bn_forward(aslp, dev, inp, st, 0, False, False, True, what + " forward")
                parts = torch.full((1024,), t.SENTINEL, device=dev)
                po = aslp._lib.PlanesOut()
                po.parts = parts.data_ptr()
                lib.aslp_device_shared(1)
                try:
                    ind = t.bn_backward(aslp, dev, inp, st, 0, x, d, None, act, True, True, what + " backward", po=po)
                finally:
                    lib.aslp_device_shared(0)
                line("%s nparts %d planes_written %d" % (what, po.nparts, po.planes_written), case.rows, case.cols, sha(act, ind, parts), state(st))
        for rows, cols, with_y in PLANES_SHAPES:
            case = ref.BnCase("planes-%dx%d" % (rows, cols), rows, cols, "coop", 0, 0, False)
            inp = ref.bn_inputs(case, seed=2000 + rows + cols)
            st = t.BnState(inp, dev)
            for k in range(2):
                what = "%s y%d call%d" % (case.name, with_y, k)
                x, d, o, xhat, act = t.bn_forward(aslp, dev, inp, st, k, not with_y, False, with_y, what + " forward")
                pl = Planes(rows, cols)
                ind = t.bn_backward(aslp, dev, inp, st, k, x, d, None, act, with_y, True, what + " backward", po=pl.po)
                line("%s nparts %d planes_written %d" % (what, pl.po.nparts, pl.po.planes_written), rows, cols, sha(o, act, ind, pl.hi, pl.lo, pl.slot), state(st))
        one = int(torch.ones(1).view(torch.int32).item())   # the activation planes' bound: a sigmoid's 1
        for rows, cols in ref.BN_STATS_SHAPES:
            case = ref.BnCase("stats-%dx%d" % (rows, cols), rows, cols, "stats", ref.bn_stats_q(rows, cols), 0, False)
            inp = ref.bn_inputs(case, seed=3000 + rows + cols)
            groups, ld = (rows + 31) // 32, cols + 4
            for planes in (False, True):
                st = t.BnState(inp, dev)
                for k in range(2):
                    x = t.Mat(dev, rows, cols, inp.x[k], float("nan"))
                    xp = torch.zeros(groups * 32, cols, device=dev)
                    xp[:rows] = x.v
                    stats = torch.full((3, groups, ld), float("nan"), dtype=torch.float64, device=dev)
                    stats[0, :, :cols] = xp.double().view(groups, 32, cols).sum(1)
                    stats[1, :, :cols] = (xp * xp).double().view(groups, 32, cols).sum(1)
                    stats[2, :, :cols] = (xp.double() * xp.double()).view(groups, 32, cols).sum(1)
                    o, act = t.Mat(dev, rows, cols), t.Mat(dev, rows, cols)
                    pl = Planes(rows, cols, one)
                    d = aslp._lib.MatrixDim(rows, cols, x.ld)
                    what = "%s planes%d call%d" % (case.name, planes, k)
                    ran = t.on_gpu(aslp, what, lambda: lib.aslp_bn_forward_stats_p(x.p, d, o.p, o.ld, t.ptr(st.scale), t.ptr(st.shift), t.ptr(st.mean), t.ptr(st.inv),
                                                                                   t.ptr(st.accm), t.ptr(st.accv), 1e-7, act.p, act.ld, t.ptr(stats), groups, ld,
                                                                                   C.byref(pl.po) if planes else None))
                    line("%s ran %d" % (what, ran), rows, cols, sha(o, act, pl.hi, pl.lo, pl.slot), state(st))
    print("bn_sweep: wrote", path)


if __name__ == "__main__":
    main()
