#!/usr/bin/env python3
"""The per-timestep recurrent kernels (csrc/gru_fused.hip, csrc/rnn_fused.hip) on the direct cases of their tests -> one line per case and
engine: which engine ran (aslp_*_step_last_pieces) and a hash of every output buffer, padding included.  Two builds that compute the same
bits write identical files:

    timeout 600 python devtools/step_sweep.py OUT.txt            (on each build)
    cmp OLD.txt NEW.txt

Shapes, seeds, buffers and the launches are the Direct classes of tests/test_gru_step_pieces_gpu.py (gru_step_ref.SHAPES, has_next 1 and 0)
and tests/test_lstm_step_split16_gpu.py (DIRECT and the two no_product / has_next = 0 cases); nothing is restated here.  Every case runs on
the fp32 instruction, with two pieces and with one piece, in this one process; Direct.run raises at the first launch that reports an error
or ran another engine than the one asked for, which ends the sweep."""
import hashlib
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else "step_sweep.txt"
    import torch
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import aslp_import
    import gru_step_ref
    import test_gru_step_pieces_gpu as gru
    import test_lstm_step_split16_gpu as lstm
    aslp = aslp_import.load()
    aslp.ops.use_torch_stream()
    dev = torch.device("cuda:0")
    sha = lambda arrays: " ".join(hashlib.sha1(a.tobytes()).hexdigest()[:16] for a in arrays)
    with open(path, "w") as out:
        for H, S in gru_step_ref.SHAPES:
            case = gru.Direct(aslp, dev, H, S)
            for has_next in (1, 0):
                for pieces in (0, 2, 1):
                    y, d = case.run(pieces, bool(has_next))
                    out.write("gru H %d S %d has_next %d [pieces %d] -> ran %d y %s d %s\n" % (H, S, has_next, pieces, aslp.lib.aslp_gru_step_last_pieces(), sha([y]), sha([d])))
        plain, first = {}, dict(no_product=True, has_next=False)
        for (Cc, S, cifg), kw in [(c, plain) for c in lstm.DIRECT] + [((20, 33, 0), first), ((132, 31, 1), first)]:
            case = lstm.Direct(aslp, dev, Cc, S, cifg, seed=100 + Cc + S, **kw)
            for split, pieces in ((0, 2), (1, 2), (1, 1)):
                ys, ds = case.run(split, pieces)
                out.write("lstm C %d S %d cifg %d %s[split %d pieces %d] -> ran %d y %s d %s\n" % (Cc, S, cifg, "no_product has_next 0 " if kw else "", split, pieces,
                                                                                                  aslp.lib.aslp_lstm_step_last_pieces(), sha(ys), sha(ds)))
    print("step_sweep: wrote", path)


if __name__ == "__main__":
    main()
