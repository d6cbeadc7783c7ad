#!/usr/bin/env python3
"""The persistent GRU recurrences (csrc/rnn_persistent.hip: aslp_gru_seq_forward / _backward) on the case list of tests/gru_seq_ref.py -> one
line per case and setting: which engine ran (aslp_gru_seq_last_pieces) and a hash of y and of d.  Two builds that compute the same bits write
identical files:

    python devtools/gru_seq_sweep.py OUT.txt            (on each build)
    cmp OLD.txt NEW.txt

Shapes, seeds and the launches are gru_seq_ref's CASES, build_case and run_on_gpu (tests/test_gru_seq_ref_cpu.py proves that the list reaches
all 12 kernels); nothing is restated here.  Every case runs under aslp_gru_seq_pieces 0, 2 and 1; ASLP_GRU_SEQ_PIECES is read once per process,
so the whole list runs once more in a fresh child with ASLP_GRU_SEQ_PIECES=2 (one child at a time).  run_on_gpu raises at the first launch
that reports an error, which ends the sweep."""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ENVS = [("api", {}), ("env", {"ASLP_GRU_SEQ_PIECES": "2"})]


def child(path, label):
    import torch
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import aslp_import
    import gru_seq_ref as ref
    aslp = aslp_import.load()
    aslp.ops.use_torch_stream()
    dev = torch.device("cuda:0")
    sha = lambda a: hashlib.sha1(a.tobytes()).hexdigest()[:16]
    inputs = [ref.build_case(c) for c in ref.CASES]
    # (what aslp_gru_seq_pieces gets, what must have run): -1 leaves the choice to the environment
    settings = [(-1, 2)] if label == "env" else [(p, p) for p in ref.PIECES]
    with open(path, "w") as out:
        for pieces, want in settings:
            for inp in inputs:
                got = ref.run_on_gpu(aslp, torch, dev, inp, pieces, want)
                out.write("%s [%s, pieces %d] -> ran %d y %s d %s\n" % (ref.case_id(inp["case"]), label, pieces, aslp.lib.aslp_gru_seq_last_pieces(), sha(got["y"]), sha(got["d"])))


def main():
    if len(sys.argv) > 3 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
        return
    path = sys.argv[1] if len(sys.argv) > 1 else "gru_seq_sweep.txt"
    with open(path, "w") as out:
        for label, env in ENVS:   # one child at a time: each holds the GPU alone
            e = dict(os.environ)
            e.pop("ASLP_GRU_SEQ_PIECES", None)
            e.update(env)
            part = "%s.%s.part" % (path, label)
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", part, label], env=e, check=True, timeout=300)
            with open(part) as f:
                out.write(f.read())
            os.remove(part)
    print("gru_seq_sweep: wrote", path)


if __name__ == "__main__":
    main()
