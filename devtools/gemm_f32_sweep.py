#!/usr/bin/env python3
"""The fp32-instruction product kernels that stage through registers (gemm_f32_mfma, csrc/gemm.hip) on the cases of their test -> one line per
call: the tile aslp_gemm_last_tile() names and a SHA-1 of every buffer the call may write, padding included.  Two builds that compute the same
bits write identical files:

    timeout 600 python devtools/gemm_f32_sweep.py OUT.txt            (on each build, on the same machine)
    cmp OLD.txt NEW.txt

First every launch of tests/test_gemm_f32_staged_gpu.py (TILES, LAYOUTS, PATHS, LAUNCHES, host, launch: tiles 1 / 7 / 12 by number; nothing is
restated here).  Then GEMM_SHAPES of tests/test_kernels_gpu.py with that test's two (alpha, beta) pairs and RAGGED of
tests/test_gemm_ragged_gpu.py in its padded storage, in all four layouts, with no tile forced and the split-fp16 products switched off: the
route the layer products of a ragged size take as shipped (LDS-DMA tiles where they are eligible, the register-staged ones behind them).
ops.sgemm raises at the first launch that reports an error, which ends the sweep."""
import hashlib
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else "gemm_f32_sweep.txt"
    import numpy as np
    import torch
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import aslp_import
    import test_gemm_f32_staged_gpu as t
    import test_gemm_ragged_gpu as ragged
    import test_kernels_gpu as kernels
    aslp = aslp_import.load()
    aslp.ops.use_torch_stream()
    dev = torch.device("cuda:0")

    def sha(*bufs):
        torch.cuda.synchronize()
        return " ".join(hashlib.sha1(b.cpu().numpy().tobytes()).hexdigest()[:16] for b in bufs)

    with open(path, "w") as out:
        def line(what, tile, hashes):
            out.write("%s -> tile %d | %s\n" % (what, tile, hashes))
            out.flush()

        for tile in t.TILES:
            for tA, tB in t.LAYOUTS:
                for name in sorted(t.PATHS):
                    for case in t.PATHS[name]:
                        for which in t.LAUNCHES:
                            for clip in (t.host(tA, tB, case).clips if which == "c" else (0.0,)):
                                ran, bufs = t.launch(aslp, dev, tile, tA, tB, case, which, clip)
                                line("forced %d tA %d tB %d %s %s launch %s clip %r %s" % (tile, tA, tB, name, tuple(case), which, clip, "+".join(sorted(bufs))),
                                     ran, sha(*(bufs[k][0] for k in sorted(bufs))))

        aslp.lib.aslp_gemm_split16(0)
        try:
            for tA, tB in t.LAYOUTS:
                for M, N, K in kernels.GEMM_SHAPES:
                    rng = np.random.default_rng(M * 7 + N * 3 + K + tA * 2 + tB)       # test_sgemm_vs_oracle's operands
                    A = kernels.T(rng.standard_normal((K, M) if tA else (M, K)).astype(np.float32), dev)
                    B = kernels.T(rng.standard_normal((N, K) if tB else (K, N)).astype(np.float32), dev)
                    C0 = rng.standard_normal((M, N)).astype(np.float32)
                    for alpha, beta in ((1.0, 0.0), (0.7, 1.3)):
                        Cd = kernels.T(C0, dev)
                        aslp.ops.sgemm(tA, tB, alpha, A, B, beta, Cd)
                        line("unforced tA %d tB %d %s alpha %g beta %g" % (tA, tB, (M, N, K), alpha, beta), aslp.lib.aslp_gemm_last_tile(), sha(Cd))
                for M, N, K in ragged.RAGGED:
                    A, B = ragged.operands(dev, tA, tB, M, N, K)
                    store, Cm = ragged.output(dev, M, N)
                    aslp.ops.sgemm(tA, tB, 1.0, A, B, 0.0, Cm)
                    line("unforced ragged tA %d tB %d %s" % (tA, tB, (M, N, K)), aslp.lib.aslp_gemm_last_tile(), sha(store))
        finally:
            aslp.lib.aslp_gemm_split16(-1)
    print("gemm_f32_sweep: wrote", path)


if __name__ == "__main__":
    main()
