#!/usr/bin/env python3
"""A fixed, seeded list of split-fp16 products (csrc/gemm_split16.hip) -> one line per case: the tile that ran (aslp_gemm_last_tile), the
per-workgroup maxima it left (aslp_gemm_last_parts) and a hash of every array the call wrote.  Two builds that choose the same tiles and
compute the same bits write identical files:

    python devtools/s16_sweep.py OUT.txt            (on each build)
    cmp OLD.txt NEW.txt

All four operand layouts, the layer shapes of the recipes and ragged ones, plain and EXTRA epilogues (planes / maxima of the output,
column sums), beta 0 and 1, one plane and two, every tile by number, and pairs (ops.sgemm_pair)."""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import aslp_import  # noqa: E402

aslp = aslp_import.load()
lib, ops, GemmEpilogue, PlanesOut = aslp.lib, aslp.ops, aslp._lib.GemmEpilogue, aslp._lib.PlanesOut
dev = torch.device("cuda:0")

# (tA, tB, M, N, K): NT = forward, NN = in-diff, TN = weight gradient, TT
SHAPES = [(0, 1, 1024, 2048, 2048), (0, 0, 1024, 2048, 2048), (1, 0, 2048, 2048, 1024),      # cfg2 hidden layers
          (0, 1, 1024, 3000, 2048), (0, 0, 1024, 2048, 3000), (1, 0, 3000, 2048, 1024),      # cfg2 output layer
          (0, 1, 256, 2048, 2048), (0, 0, 256, 2048, 2048), (1, 0, 2048, 2048, 256),         # minibatch 256
          (0, 1, 256, 2048, 440), (1, 0, 2048, 440, 256), (0, 0, 256, 2048, 3000),           # ... its 440-input and output layers
          (0, 1, 1920, 2048, 512), (0, 0, 1920, 512, 2048), (1, 0, 2048, 512, 1920),         # LC-BLSTM batched products
          (0, 1, 2048, 2048, 2048), (0, 1, 4096, 2048, 2048), (0, 1, 4096, 4096, 4096), (1, 0, 4096, 4096, 4096),
          (0, 1, 1920, 3000, 1024), (1, 1, 512, 640, 768), (1, 1, 2048, 2048, 1024),
          (0, 1, 1000, 3000, 440), (0, 0, 132, 260, 68), (1, 0, 436, 128, 2052), (0, 1, 192, 1920, 1028), (1, 0, 196, 332, 100),
          (1, 1, 260, 132, 1028), (0, 1, 1088, 1984, 1028), (0, 0, 1004, 2052, 100), (1, 0, 1348, 1092, 68)]
FORCED = (304, 308, 311, 312, 328, 351)
FORCED_SHAPES = [(0, 1, 1024, 2048, 2048), (0, 0, 1024, 2048, 2048), (1, 0, 2048, 2048, 1024), (1, 1, 512, 640, 768), (0, 1, 1000, 3000, 440),
                 (1, 0, 436, 128, 2052), (0, 1, 192, 1920, 1028)]


def digest(*tensors):
    h = hashlib.sha1()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def operands(tA, tB, M, N, K, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    A = torch.randn((K, M) if tA else (M, K), device=dev, generator=g)
    B = torch.randn((N, K) if tB else (K, N), device=dev, generator=g) * 0.05
    C0 = torch.randn(M, N, device=dev, generator=g)
    return A, B, C0, g


def one(out, tA, tB, M, N, K, planes, beta, extra, tile):
    A, B, C0, g = operands(tA, tB, M, N, K, 1000 * tA + 2000 * tB + M + 3 * N + 7 * K)
    Cm = C0.clone()
    written = [Cm]
    ep = None
    if extra:   # what the layers ask for: forward -> bias, sigmoid output and its planes + max |C|; in-diff -> max |C|; weight gradient -> the fused step
        ld = (N + 63) // 64 * 64   # planes as a producer kernel takes them: [rows rounded to 64][ld]
        hi, lo = (torch.full(((M + 63) // 64 * 64, ld), 7.0, dtype=torch.float16, device=dev) for _ in range(2))
        wmax, cmax = (torch.full((4096,), -1.0, device=dev) for _ in range(2))
        if tA:
            W = torch.randn(M, N, device=dev, generator=g)
            bc, b = torch.randn(M, device=dev, generator=g), torch.randn(M, device=dev, generator=g)
            slot = torch.tensor([W.abs().max().item() + 0.01 * 60.0], dtype=torch.float32, device=dev)
            po = PlanesOut(hi.data_ptr(), lo.data_ptr(), ld, slot.data_ptr(), None, 0, 0)
            colsum = (bc.data_ptr(), 0.9, b.data_ptr(), -0.02) if not tB else (None, 0.0, None, 0.0)
            ep = GemmEpilogue(None, 60.0, W.data_ptr(), N, -0.01, None, 0, 0, *colsum, None, 0, None, 0, po, 1, wmax.data_ptr(), cmax.data_ptr(), None, None, 0)
            written += [W, bc, b, hi, lo, wmax, cmax]
        elif tB:
            bias, act = torch.randn(N, device=dev, generator=g), torch.zeros(M, N, device=dev)
            slot = torch.tensor([1.0], dtype=torch.float32, device=dev)
            po = PlanesOut(hi.data_ptr(), lo.data_ptr(), ld, slot.data_ptr(), None, 0, 0)
            ep = GemmEpilogue(bias.data_ptr(), 0.0, None, 0, 0.0, act.data_ptr(), N, 1, None, 0.0, None, 0.0, None, 0, None, 0, po, 2, None, cmax.data_ptr(), None, None, 0)
            written += [act, hi, lo, cmax]
        else:
            ep = GemmEpilogue(None, 0.0, None, 0, 0.0, None, 0, 0, None, 0.0, None, 0.0, None, 0, None, 0, PlanesOut(), 0, None, cmax.data_ptr(), None, None, 0)
            written += [cmax]
    lib.aslp_gemm_split16_tile(tile if tile else -1)
    with ops.operand_planes(planes):
        ops.sgemm(tA, tB, 1.0, A, B, beta, Cm, ep)
    lib.aslp_gemm_split16_tile(-1)
    out.write("sgemm %d%d %dx%dx%d planes=%d beta=%g extra=%d forced=%d -> tile %d parts %d %s\n" %
              (tA, tB, M, N, K, planes, beta, extra, tile, lib.aslp_gemm_last_tile(), lib.aslp_gemm_last_parts(), digest(*written)))


def pair(out, tA, tB, M, N, K, planes, beta):
    A0, B0, C0, _ = operands(tA, tB, M, N, K, 5 + M + N + K)
    A1, B1, C1, _ = operands(tA, tB, M, N, K, 6 + M + N + K)
    with ops.operand_planes(planes):
        ops.sgemm_pair(tA, tB, 1.0, A0, A1, B0, B1, beta, C0, C1)
    out.write("pair  %d%d %dx%dx%d planes=%d beta=%g -> tile %d parts %d %s\n" %
              (tA, tB, M, N, K, planes, beta, lib.aslp_gemm_last_tile(), lib.aslp_gemm_last_parts(), digest(C0, C1)))


def main():
    ops.use_torch_stream()
    lib.aslp_gemm_split16(1)
    with open(sys.argv[1] if len(sys.argv) > 1 else "s16_sweep.txt", "w") as out:
        for planes in (2, 1):
            for (tA, tB, M, N, K) in SHAPES:
                big = M * N * K > 2 ** 34
                for beta in ((0.0,) if big else (0.0, 1.0)):
                    for extra in ((0,) if big else (0, 1)):
                        one(out, tA, tB, M, N, K, planes, beta, extra, 0)
            for shape in FORCED_SHAPES:
                for tile in FORCED:
                    for extra in (0, 1):
                        one(out, *shape, planes, 0.0, extra, tile + 100 if planes == 1 and extra else tile)
            for (tA, tB, M, N, K) in [(0, 1, 1920, 2048, 512), (0, 0, 1920, 512, 2048), (1, 0, 2048, 512, 1920), (0, 1, 256, 2048, 2048), (0, 1, 196, 332, 100)]:
                for beta in (0.0, 1.0):
                    pair(out, tA, tB, M, N, K, planes, beta)
    torch.cuda.synchronize()
    lib.aslp_gemm_split16(-1)
    print("s16_sweep: wrote", sys.argv[1] if len(sys.argv) > 1 else "s16_sweep.txt")


if __name__ == "__main__":
    main()
