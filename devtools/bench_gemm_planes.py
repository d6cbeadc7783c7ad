"""Two-plane against one-plane layer products (aslp_gemm_operand_planes), interleaved A-B-A on a warm chip, from prepared planes as the
training step issues them.  The chip is warmed for about a second first and every timing is a window of `reps` calls behind 50 untimed
ones (shorter warm-ups bias whatever is timed first).  A second table times the one-plane 64 x 128 tile (408) against the 128 x 128 one (411)
on grids where the dispatcher may pick either.
usage: python devtools/bench_gemm_planes.py [reps]"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aslp_import

aslp = aslp_import.load()
aslp.ops.use_torch_stream()
dev = torch.device("cuda:0")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
SHAPES = [("NT", 0, 1, 1024, 2048, 2048), ("NN", 0, 0, 1024, 2048, 2048), ("TN", 1, 0, 2048, 2048, 1024), ("NT", 0, 1, 1024, 3000, 2048),
          ("NT", 0, 1, 256, 2048, 2048), ("NN", 0, 0, 256, 2048, 2048), ("TN", 1, 0, 2048, 2048, 256), ("NT", 0, 1, 256, 3000, 2048)]
TILE_SHAPES = [("NT", 0, 1, 2048, 2048, 2048), ("NT", 0, 1, 4096, 2048, 2048), ("NT", 0, 1, 4096, 4096, 4096)]


def timed(planes, tA, tB, A, pa, B, pb, C, tile=-1):
    aslp.ops.set_operand_planes(planes)
    aslp.lib.aslp_gemm_split16_tile(tile)
    for _ in range(50):
        aslp.ops.sgemm_planes(tA, tB, 1.0, A, pa, B, pb, 0.0, C)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        aslp.ops.sgemm_planes(tA, tB, 1.0, A, pa, B, pb, 0.0, C)
    e1.record()
    e1.synchronize()
    aslp.lib.aslp_gemm_split16_tile(-1)
    return 1e3 * e0.elapsed_time(e1) / reps, aslp.lib.aslp_gemm_last_tile()


def operands(tA, tB, M, N, K):
    A = torch.randn((K, M) if tA else (M, K), device=dev)
    B = torch.randn((N, K) if tB else (K, N), device=dev)
    return A, aslp.ops.Planes(A), B, aslp.ops.Planes(B), torch.zeros(M, N, device=dev)


A, pa, B, pb, C = operands(0, 1, 2048, 2048, 2048)
t0 = time.time()
while time.time() - t0 < 1.5:      # clock ramp
    for _ in range(200):
        aslp.ops.sgemm_planes(0, 1, 1.0, A, pa, B, pb, 0.0, C)
    torch.cuda.synchronize()

print("layout M N K : us/call 2 planes (tile) | 1 plane (tile) | 2 planes again | 1 plane / slower 2-plane reading .. / faster")
for name, tA, tB, M, N, K in SHAPES:
    A, pa, B, pb, C = operands(tA, tB, M, N, K)
    t2a, c2 = timed(2, tA, tB, A, pa, B, pb, C)
    t1, c1 = timed(1, tA, tB, A, pa, B, pb, C)
    t2b, _ = timed(2, tA, tB, A, pa, B, pb, C)
    print("%s %d %d %d : %.1f (%d) | %.1f (%d) | %.1f | %.2f .. %.2f" % (name, M, N, K, t2a, c2, t1, c1, t2b, t1 / max(t2a, t2b), t1 / min(t2a, t2b)))
print("one plane, tile by number: layout M N K : us/call 408 | 411 | 408 again | heuristic (tile)")
for name, tA, tB, M, N, K in TILE_SHAPES:
    A, pa, B, pb, C = operands(tA, tB, M, N, K)
    a, ca = timed(1, tA, tB, A, pa, B, pb, C, 408)
    b, cb = timed(1, tA, tB, A, pa, B, pb, C, 411)
    a2, _ = timed(1, tA, tB, A, pa, B, pb, C, 408)
    h, ch = timed(1, tA, tB, A, pa, B, pb, C)
    assert (ca, cb) == (408, 411), (ca, cb)
    print("%s %d %d %d : %.1f | %.1f | %.1f | %.1f (%d)" % (name, M, N, K, a, b, a2, h, ch))
aslp.ops.set_operand_planes(-1)
del pa, pb
