#!/usr/bin/env python3
"""A fixed, seeded list of persistent LSTM recurrences (csrc/rnn_persistent.hip: aslp_lstm_seq_forward / _backward) -> one line per case and
pass: which kernel family ran (aslp_lstm_seq_last_pieces, aslp_lstm_seq_last_dmax) and a hash of every buffer the call wrote (y; d,
grad_partial and the dmax parts).  Two builds that compute the same bits write identical files:

    python devtools/lstm_seq_sweep.py OUT.txt            (on each build)
    cmp OLD.txt NEW.txt

Cells 68 .. 512 (a partial last workgroup, both sizes of every instantiation family, the wave-slice tail), 5 / 9 / 32 streams (a partial chain,
one full + one partial, eight chains), T = 1 (no hand-off), 2 and 6 (wraps the backward ring of 4), one and two directions, CIFG, ragged
seq_lengths with streams of length 0 and 1, w_first with k_first 40 and 256, skip_first_product, grad_partial on and off, a stream window.
Every case runs under the default switches, aslp_lstm_split16(0) and aslp_lstm_operand_pieces(1); the environment switches are read once per
process, so the whole list runs again in a fresh child per setting (one at a time): ASLP_LSTM_FAST_ACT=0, ASLP_LSTM_WAVE_COLLECT=0,
ASLP_LSTM_READ_AHEAD=0."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

ENVS = [("default", {}), ("fast_act0", {"ASLP_LSTM_FAST_ACT": "0"}), ("wave_collect0", {"ASLP_LSTM_WAVE_COLLECT": "0"}),
        ("read_ahead0", {"ASLP_LSTM_READ_AHEAD": "0"})]
SWITCHES = [("default", -1, -1), ("split16=0", 0, -1), ("pieces=1", -1, 1)]   # (label, aslp_lstm_split16, aslp_lstm_operand_pieces)
# (C, S, T, ndir, cifg, ragged, k_first (0: no w_first), skip_first_product, grad_partial, (s_begin, s_count))
CASES = [(68, 5, 1, 1, 0, 0, 0, 0, 1, (0, 0)),
         (68, 9, 6, 2, 1, 1, 40, 0, 1, (0, 0)),
         (128, 9, 2, 2, 0, 1, 40, 0, 0, (0, 0)),
         (128, 32, 6, 1, 1, 0, 0, 1, 1, (0, 0)),
         (132, 32, 6, 2, 0, 1, 0, 0, 1, (0, 0)),
         (132, 5, 2, 1, 1, 0, 256, 0, 0, (0, 0)),
         (260, 9, 6, 1, 0, 1, 256, 0, 1, (0, 0)),
         (260, 32, 6, 2, 1, 1, 40, 0, 1, (8, 16)),
         (512, 32, 6, 2, 0, 1, 256, 0, 1, (0, 0)),
         (512, 5, 2, 1, 1, 0, 0, 1, 0, (0, 0)),
         (512, 9, 1, 2, 0, 1, 40, 0, 1, (3, 5))]


def child(path, label):
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import aslp_import
    aslp = aslp_import.load()
    lib, ops = aslp.lib, aslp.ops
    Seq = aslp._lib.Seq   # the structures and the signatures of aslp_lstm_seq_* live with the binding (kaldi-aslp_amd/_lib.py)
    dev = torch.device("cuda:0")
    ops.use_torch_stream()

    def digest(*tensors):
        h = hashlib.sha1()
        for t in tensors:
            h.update(t.detach().contiguous().cpu().numpy().tobytes())
        return h.hexdigest()[:16]

    def one(out, sw, case):
        Cc, S, T, ndir, cifg, ragged, k_first, skip, gp, (s_begin, s_count) = case
        G = 3 if cifg else 4
        ld = (G + 3) * Cc                      # [gates | c | h | m]
        g = torch.Generator(device=dev).manual_seed(7 * Cc + 11 * S + 13 * T + ndir + 2 * cifg + k_first + 1000 * (ragged + 2 * skip + 4 * gp) + 10000 * s_begin + 100000 * s_count)
        rnd = lambda *shape, scale=1.0: torch.randn(*shape, device=dev, generator=g) * scale
        a = Seq()
        a.ndir, a.ld, a.ldw, a.T, a.S, a.C, a.cifg, a.s_begin, a.s_count = ndir, ld, Cc, T, S, Cc, cifg, s_begin, s_count
        keep, ys, ds = [], [], []
        lens = torch.tensor([(0, 1, T, max(T - 1, 0))[s % 4] if ragged else T for s in range(S)], dtype=torch.int32, device=dev)
        for d in range(ndir):
            y = torch.zeros((T + 2) * S, ld, device=dev)
            lib.aslp_lstm_seq_fill(y.data_ptr(), ld, T, S, (G + 2) * Cc, Cc)   # before anything is stored into it
            y.view(T + 2, S, ld)[1:T + 1, :, :G * Cc] = rnd(T, S, G * Cc)       # x-part + bias
            hist = 0 if d == 0 else T + 1                                       # the row block the recursion starts from
            y.view(T + 2, S, ld)[hist, :, G * Cc:] = rnd(S, 3 * Cc, scale=0.5)  # c, h, m of the history
            if k_first:
                y.view(T + 2, S, ld)[hist, :, :k_first] = rnd(S, k_first, scale=0.5)   # r(0): columns [0, k_first) of the history row block
            dd = torch.zeros((T + 2) * S, ld, device=dev)
            dd.view(T + 2, S, ld)[1:T + 1, :, (G + 2) * Cc:] = rnd(T, S, Cc)    # dL/dm from the layer above
            w, wf = rnd(G * Cc, Cc, scale=0.08), rnd(G * Cc, max(k_first, 4), scale=0.08)
            pi, pf, po = rnd(Cc, scale=0.3), rnd(Cc, scale=0.3), rnd(Cc, scale=0.3)
            q = a.dir[d]
            q.y, q.d, q.w, q.peep_i, q.peep_f, q.peep_o = y.data_ptr(), dd.data_ptr(), w.data_ptr(), pi.data_ptr(), pf.data_ptr(), po.data_ptr()
            q.seq_lengths = lens.data_ptr() if ragged else None
            q.reverse, q.skip_first_product = d, skip
            if k_first:
                q.w_first, q.ldw_first, q.k_first, q.col_first = wf.data_ptr(), wf.shape[1], k_first, 0
            keep += [w, wf, pi, pf, po]; ys.append(y); ds.append(dd)
        part = torch.full((8 * 7, Cc), -1.0, device=dev)
        dmax = [torch.full((256,), -1.0, device=dev) for _ in range(2)]
        if gp:
            a.grad_partial, a.grad_ld = part.data_ptr(), Cc
        for d in range(ndir):
            a.dmax_parts[d] = dmax[d].data_ptr()
        tag = "C=%d S=%d T=%d ndir=%d cifg=%d ragged=%d k_first=%d skip=%d gp=%d window=%d+%d [%s]" % (Cc, S, T, ndir, cifg, ragged, k_first, skip, gp, s_begin, s_count, sw)
        for backward, name in ((0, "fwd"), (1, "bwd")):
            if not lib.aslp_lstm_seq_supported(C.byref(a), backward):
                out.write("%s %s -> not supported\n" % (name, tag))   # (probed per pass: the other pass may still run)
                if not backward:   # ... on finite activations in place of the ones the forward pass would have left
                    for y in ys:
                        y.view(T + 2, S, ld)[1:T + 1] = torch.rand(T, S, ld, device=dev, generator=g)
                continue
            (lib.aslp_lstm_seq_backward if backward else lib.aslp_lstm_seq_forward)(C.byref(a))
            torch.cuda.synchronize()
            aslp._lib.check_error()
            written = ds + [part] + dmax if backward else ys
            out.write("%s %s -> pieces %d dmax %d %s\n" % (name, tag, lib.aslp_lstm_seq_last_pieces(), lib.aslp_lstm_seq_last_dmax() if backward else 0, digest(*written)))
        del keep

    with open(path, "w") as out:
        for sw, split, pieces in SWITCHES:
            lib.aslp_lstm_split16(split)
            ops.set_lstm_operand_pieces(pieces)
            for case in CASES:
                one(out, "%s, %s" % (label, sw), case)
        lib.aslp_lstm_split16(-1)
        ops.set_lstm_operand_pieces(-1)


def main():
    if len(sys.argv) > 3 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
        return
    path = sys.argv[1] if len(sys.argv) > 1 else "lstm_seq_sweep.txt"
    with open(path, "w") as out:
        for label, env in ENVS:   # one child at a time: each holds the GPU alone
            e = dict(os.environ)
            for k in ("ASLP_LSTM_FAST_ACT", "ASLP_LSTM_WAVE_COLLECT", "ASLP_LSTM_READ_AHEAD", "ASLP_LSTM_SPLIT_F16", "ASLP_LSTM_PIECES"):
                e.pop(k, None)
            e.update(env)
            part = "%s.%s.part" % (path, label)
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", part, label], env=e, check=True, timeout=300)
            with open(part) as f:
                out.write(f.read())
            os.remove(part)
    print("lstm_seq_sweep: wrote", path)


if __name__ == "__main__":
    main()
