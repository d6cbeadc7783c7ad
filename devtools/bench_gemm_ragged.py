"""Layer products at sizes that are no multiple of 4 with aslp_gemm_split16_ragged off (as shipped: the fp32 instruction's register-staged
kernel) and on (the split-fp16 kernels, behind the conversion kernels' ragged forms), interleaved off - on - off on a warm chip, and each
shape's multiple-of-4 neighbour with the switch on.  The chip is warmed for about a second first and every timing is a window of `reps`
calls between two events behind 30 untimed ones.  "inside": aslp_sgemm_ex converts both operands in the call (a maximum pass and a
conversion pass, or the single launch); "planes": from prepared planes, as the training step issues its products.  Matrices lie in rows
padded to a multiple of 4 floats, as CuMatrix lays them out.  Both plane counts.
usage: python devtools/bench_gemm_ragged.py [reps] [out.txt]"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aslp_import

aslp = aslp_import.load()
aslp.ops.use_torch_stream()
dev = torch.device("cuda:0")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 500
out_path = sys.argv[2] if len(sys.argv) > 2 else None
# (layout, transA, transB, M, N, K, the neighbour's M, N, K): the output layer of a 3001-pdf tree in its three products, a 429-wide input
# in the two products that read it, an utterance of 1001 frames
SHAPES = [("NT", 0, 1, 1024, 3001, 2048, 1024, 3000, 2048), ("NN", 0, 0, 1024, 2048, 3001, 1024, 2048, 3000),
          ("TN", 1, 0, 3001, 2048, 1024, 3000, 2048, 1024), ("NT", 0, 1, 1024, 2048, 429, 1024, 2048, 428),
          ("TN", 1, 0, 2048, 429, 1024, 2048, 428, 1024), ("NT", 0, 1, 1001, 2048, 2048, 1000, 2048, 2048)]
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def padded(rows, cols, fill=None):
    store = torch.zeros(rows, (cols + 15) // 16 * 16, device=dev)
    view = store[:, :cols]
    if fill is None:
        view.copy_(torch.randn(rows, cols, device=dev))
    return view


def operands(tA, tB, M, N, K):
    return padded(*((K, M) if tA else (M, K))), padded(*((N, K) if tB else (K, N))), padded(M, N, 0.0)


def timed(on, planes, tA, tB, A, B, C, prepared):
    aslp.ops.set_split16_ragged(on)
    aslp.ops.set_operand_planes(planes)
    pa, pb = (aslp.ops.Planes(A), aslp.ops.Planes(B)) if prepared else (None, None)
    for _ in range(30):
        aslp.ops.sgemm_planes(tA, tB, 1.0, A, pa, B, pb, 0.0, C)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        aslp.ops.sgemm_planes(tA, tB, 1.0, A, pa, B, pb, 0.0, C)
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps, aslp.lib.aslp_gemm_last_tile()


A, B, C = operands(0, 1, 2048, 2048, 2048)
t0 = time.time()
while time.time() - t0 < 1.5:      # clock ramp
    for _ in range(200):
        aslp.ops.sgemm(0, 1, 1.0, A, B, 0.0, C)
    torch.cuda.synchronize()

say("us per call, %d calls per window.  off / off again: aslp_gemm_split16_ragged(0); inside / planes: (1); nb: the multiple-of-4 neighbour under (1)" % reps)
say("planes layout M N K : off (tile) | inside (tile) | planes (tile) | off again | nb M N K inside | nb planes (tile) | inside / slower off .. / faster off | planes / nb planes")
for planes in (2, 1):
    for name, tA, tB, M, N, K, M4, N4, K4 in SHAPES:
        A, B, C = operands(tA, tB, M, N, K)
        off_a, tile_off = timed(0, planes, tA, tB, A, B, C, False)
        ins, tile_in = timed(1, planes, tA, tB, A, B, C, False)
        pre, tile_pre = timed(1, planes, tA, tB, A, B, C, True)
        off_b, _ = timed(0, planes, tA, tB, A, B, C, False)
        A4, B4, C4 = operands(tA, tB, M4, N4, K4)
        nb_in, _ = timed(1, planes, tA, tB, A4, B4, C4, False)
        nb_pre, tile_nb = timed(1, planes, tA, tB, A4, B4, C4, True)
        say("%d %s %d %d %d : %.1f (%d) | %.1f (%d) | %.1f (%d) | %.1f | %d %d %d %.1f | %.1f (%d) | %.2f .. %.2f | %.2f" %
            (planes, name, M, N, K, off_a, tile_off, ins, tile_in, pre, tile_pre, off_b, M4, N4, K4, nb_in, nb_pre, tile_nb,
             ins / max(off_a, off_b), ins / min(off_a, off_b), pre / nb_pre))
aslp.ops.set_operand_planes(-1)
aslp.ops.set_split16_ragged(-1)
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
