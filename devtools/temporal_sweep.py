#!/usr/bin/env python3
"""The temporal filter kernels (csrc/temporal.hip) on the cases of their test -> one line per call: the path the library names
(aslp_rowconv_path / aslp_fsmn_path) and a SHA-1 of every buffer the call may write, padding included.  Two builds that compute the same bits
write identical files:

    timeout 600 python devtools/temporal_sweep.py OUT.txt            (on each build, on the same machine)
    cmp OLD.txt NEW.txt

Shapes, seeds, leading dimensions, buffers and the launches are those of tests/test_temporal_kernels_gpu.py (temporal_ref.RC_CASES, FSMN_CASES,
rc_inputs, fsmn_inputs, rc_ld; Mat, vec, rc_mats, rc_out, on_gpu); nothing is restated here.  Per case the test's own two consecutive calls
(they carry the parameters and the momentum buffer) of forward + backward, with the folded step and without; without it also the stand-alone
entry points aslp_rowconv_backward, aslp_rowconv_wgrad, aslp_fsmn_coef_grad and the reversed aslp_fsmn_filter.  on_gpu raises at the first
launch that reports an error, which ends the sweep."""
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else "temporal_sweep.txt"
    import numpy as np
    import torch
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import aslp_import
    import temporal_ref as ref
    import test_temporal_kernels_gpu as t
    aslp = aslp_import.load()
    aslp.ops.use_torch_stream()
    dev = torch.device("cuda:0")
    lib = aslp.lib

    def sha(*mats):
        torch.cuda.synchronize()
        return " ".join(hashlib.sha1(m.buf.cpu().numpy().tobytes()).hexdigest()[:16] for m in mats)

    with open(path, "w") as out:
        def line(what, where, hashes):
            out.write("%s -> %s | %s\n" % (what, where, hashes))
            out.flush()

        for c in ref.RC_CASES:
            inp = ref.rc_inputs(c)
            lens = torch.from_numpy(inp.lens).to(dev)
            lp = C.c_void_p(lens.data_ptr())
            shape = (c.D, c.K + 1)
            blank = lambda: t.vec(dev, np.full(shape, t.SENTINEL, np.float32))
            for update in (0, 1):
                w, wc = t.vec(dev, inp.w), t.vec(dev, inp.w_corr)
                for k in range(2):
                    what = "rowconv %s update%d call%d" % (c.name, update, k)
                    x, od = t.rc_mats(dev, inp, k)
                    y, idf, wd = t.rc_out(dev, c), t.rc_out(dev, c), blank()
                    fwd = "ring %d" % lib.aslp_rowconv_path(c.D, c.K, y.ld, x.ld, 0, y.p, x.p, None)
                    bwd = "ring %d" % lib.aslp_rowconv_path(c.D, c.K, idf.ld, x.ld, od.ld, idf.p, x.p, od.p)
                    t.on_gpu(aslp, what + " forward", lambda: lib.aslp_rowconv_forward(y.p, y.ld, x.p, x.ld, w.p, c.D, c.K, c.T, c.S, lp))
                    line(what + " forward", fwd, sha(y))
                    t.on_gpu(aslp, what + " backward", lambda: lib.aslp_rowconv_backward_fused(idf.p, idf.ld, wd.p, x.p, x.ld, od.p, od.ld, w.p, c.D, c.K, c.T, c.S,
                                                                                               lp, wc.p, ref.MMT, ref.LR, update))
                    line(what + " backward", bwd, sha(idf, wd, w, wc))
                    if not update:
                        idf3, wd3 = t.rc_out(dev, c), blank()
                        t.on_gpu(aslp, what + " plain backward", lambda: lib.aslp_rowconv_backward(idf3.p, idf3.ld, od.p, od.ld, w.p, c.D, c.K, c.T, c.S, lp))
                        line(what + " aslp_rowconv_backward", "plain", sha(idf3))
                        t.on_gpu(aslp, what + " plain wgrad", lambda: lib.aslp_rowconv_wgrad(wd3.p, x.p, x.ld, od.p, od.ld, c.D, c.K, c.T, c.S, lp))
                        line(what + " aslp_rowconv_wgrad", "plain", sha(wd3))

        for c in ref.FSMN_CASES:
            inp = ref.fsmn_inputs(c)
            Cn, D, T = c.P + c.F + 1, c.D, c.T
            for lr in (0.0, ref.LR):
                coef = t.Mat(dev, Cn, D, D + 3, inp.coef)
                for k in range(2):
                    what = "fsmn %s lr%g call%d" % (c.name, lr, k)
                    clip = inp.clip[k]
                    x, od = t.Mat(dev, T, D, D + 4, inp.x[k], t.NAN), t.Mat(dev, T, D, D + 2, inp.od[k], t.NAN)
                    y, idf, corr = t.Mat(dev, T, D, D + 1), t.Mat(dev, T, D, D + 5), t.Mat(dev, Cn, D, D + 1)
                    fwd = "tiled %d" % lib.aslp_fsmn_path(D, c.P, c.F, T, D + 5, 0)
                    bwd = "fused %d" % lib.aslp_fsmn_path(D, c.P, c.F, T, D + 5, 1)
                    t.on_gpu(aslp, what + " forward", lambda: lib.aslp_fsmn_filter(y.p, y.ld, x.p, x.ld, coef.p, coef.ld, D, c.P, c.F, T, 0))
                    line(what + " forward", fwd, sha(y))
                    t.on_gpu(aslp, what + " backward", lambda: lib.aslp_fsmn_backward(idf.p, idf.ld, corr.p, corr.ld, coef.p, coef.ld, x.p, x.ld, od.p, od.ld, D, c.P,
                                                                                      c.F, T, clip, lr))
                    line(what + " backward", bwd, sha(idf, corr, coef))
                    if lr == 0.0:
                        corr3, idf3 = t.Mat(dev, Cn, D, D + 2), t.Mat(dev, T, D, D + 3)
                        t.on_gpu(aslp, what + " coef_grad", lambda: lib.aslp_fsmn_coef_grad(corr3.p, corr3.ld, x.p, x.ld, od.p, od.ld, D, c.P, c.F, T, clip))
                        line(what + " aslp_fsmn_coef_grad", "separate", sha(corr3))
                        t.on_gpu(aslp, what + " reversed filter", lambda: lib.aslp_fsmn_filter(idf3.p, idf3.ld, od.p, od.ld, coef.p, coef.ld, D, c.P, c.F, T, 1))
                        line(what + " reversed aslp_fsmn_filter", fwd, sha(idf3))
    print("temporal_sweep: wrote", path)


if __name__ == "__main__":
    main()
