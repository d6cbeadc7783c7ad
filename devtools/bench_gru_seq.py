"""The persistent GRU recurrences alone (aslp_gru_seq_forward / _backward through the C ABI) at H cells, S streams, T frames: device time per
launch and per timestep under aslp_gru_seq_pieces 0 / 2 / 0 / 1 / 0 (old / new / old, one process, one box), device events around each
launch, the buffers put back before every launch outside the timed window.
Usage: python devtools/bench_gru_seq.py [H] [S] [T] [launches per round]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import aslp_import

aslp = aslp_import.load(); aslp.ops.use_torch_stream()
lib = aslp.lib
H = int(sys.argv[1]) if len(sys.argv) > 1 else 512
S = int(sys.argv[2]) if len(sys.argv) > 2 else 32
T = int(sys.argv[3]) if len(sys.argv) > 3 else 60
N = int(sys.argv[4]) if len(sys.argv) > 4 else 30
dev = torch.device("cuda:0")
g = torch.Generator(device="cpu"); g.manual_seed(1)
rnd = lambda *shape, scale=1.0: (torch.randn(*shape, generator=g) * scale).to(dev)
ld = 5 * H
x = rnd(T, S, 3 * H)
h0 = rnd(S, H, scale=0.5)
dh = rnd(T, S, H)
w_zr, w_m = rnd(2 * H, H, scale=0.04), rnd(H, H, scale=0.04)
w_zr_t, w_m_t = w_zr.t().contiguous(), w_m.t().contiguous()
y = torch.zeros((T + 2) * S, ld, device=dev)
d = torch.zeros((T + 2) * S, ld, device=dev)
yv, dv = y.view(T + 2, S, ld), d.view(T + 2, S, ld)


def args(backward):
    a = aslp._lib.GruSeq()
    a.y, a.d = y.data_ptr(), d.data_ptr() if backward else None
    a.w_zr, a.w_m = (w_zr_t if backward else w_zr).data_ptr(), (w_m_t if backward else w_m).data_ptr()
    a.ldw_zr, a.ldw_m, a.ld, a.T, a.S, a.H = (2 * H if backward else H), H, ld, T, S, H
    return a


def one(backward):
    """one launch, buffers prepared before the first event; -> device ms"""
    if not backward:
        lib.aslp_lstm_seq_fill(y.data_ptr(), ld, T, S, 3 * H, 2 * H)
        yv[1:T + 1, :, :3 * H] = x
        yv[0, :, 4 * H:] = h0
    else:
        lib.aslp_lstm_seq_fill(d.data_ptr(), ld, T, S, 0, 3 * H)
        dv[1:T + 1, :, 3 * H:4 * H] = 0
        dv[1:T + 1, :, 4 * H:] = dh
    a = args(backward)
    assert lib.aslp_gru_seq_supported(C.byref(a), backward) == 1
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    (lib.aslp_gru_seq_backward if backward else lib.aslp_gru_seq_forward)(C.byref(a))
    e1.record()
    torch.cuda.synchronize()
    aslp._lib.check_error()
    return e0.elapsed_time(e1)


print("gru_seq H=%d S=%d T=%d, %d launches per round; us per timestep: median (min .. max) over the round's launches" % (H, S, T, N))
for pieces in (0, 2, 0, 1, 0):
    lib.aslp_gru_seq_pieces(pieces)
    row = []
    for backward in (0, 1):
        for _ in range(3):
            one(0); one(1)       # (a backward launch reads what the forward one left)
        ts = []
        for _ in range(N):
            if backward:
                one(0)
            ts.append(one(backward) * 1e3 / T)
        assert lib.aslp_gru_seq_last_pieces() == pieces
        ts.sort()
        row.append("%s %6.2f (%6.2f .. %6.2f)" % ("bwd" if backward else "fwd", ts[len(ts) // 2], ts[0], ts[-1]))
    print("pieces %d: %s" % (pieces, "   ".join(row)))
lib.aslp_gru_seq_pieces(-1)
