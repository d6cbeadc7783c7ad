"""The tile / split-K choice of the split-fp16 products (csrc/gemm_split16.hip s16_plan) as a table, without a device:
aslp_gemm_split16_plan launches nothing.  The expected values are what the products of these shapes ran on before the choice became a
function of its own (devtools/s16_sweep.py on an MI355X records the same numbers from real launches)."""
import ctypes as C

import pytest

A16 = 0x1000   # a 16-byte aligned address the planner only tests for NULL and alignment


def epilogue(aslp, kind, N):
    """what the layers ask of their products (devtools/s16_sweep.py): forward -> bias, sigmoid output with its planes, max |C|;
    in-diff -> max |C|; weight gradient -> the fused step with the planes of W, both maxima and the bias gradient"""
    E, P = aslp._lib.GemmEpilogue, aslp._lib.PlanesOut
    if kind == "fwd":
        return E(A16, 0.0, None, 0, 0.0, A16, N, 1, None, 0.0, None, 0.0, None, 0, None, 0, P(A16, A16, N, A16, None, 0, 0), 2, None, A16, None, None, 0)
    if kind == "indiff":
        return E(None, 0.0, None, 0, 0.0, None, 0, 0, None, 0.0, None, 0.0, None, 0, None, 0, P(), 0, None, A16, None, None, 0)
    if kind == "wgrad":
        return E(None, 60.0, A16, N, -0.01, None, 0, 0, A16, 0.9, A16, -0.02, None, 0, None, 0, P(A16, A16, N, A16, None, 0, 0), 1, A16, A16, None, None, 0)
    return None


# (transA, transB, M, N, K, epilogue kind, tile asked for) -> (tile, K chunks) with two planes, (tile, K chunks) with one
TABLE = [
    # cfg2 (minibatch 1024): hidden and output layers in the three layouts
    ((0, 1, 1024, 2048, 2048, None, 0), (308, 0), (408, 0)), ((0, 1, 1024, 2048, 2048, "fwd", 0), (308, 0), (408, 0)),
    ((0, 0, 1024, 2048, 2048, None, 0), (308, 0), (408, 0)), ((0, 0, 1024, 2048, 2048, "indiff", 0), (308, 0), (408, 0)),
    ((1, 0, 2048, 2048, 1024, None, 0), (328, 0), (408, 0)), ((1, 0, 2048, 2048, 1024, "wgrad", 0), (328, 0), (408, 0)),
    ((0, 1, 1024, 3000, 2048, None, 0), (308, 0), (408, 0)), ((0, 0, 1024, 2048, 3000, None, 0), (308, 0), (408, 0)),
    ((1, 0, 3000, 2048, 1024, None, 0), (308, 0), (408, 0)), ((1, 0, 3000, 2048, 1024, "wgrad", 0), (308, 0), (408, 0)),
    # minibatch 256: 32 x 64 tiles with the whole reduction; the 440-input layer only when it has planes / maxima to leave
    ((0, 1, 256, 2048, 2048, None, 0), (304, 0), (404, 0)), ((0, 0, 256, 2048, 2048, "indiff", 0), (304, 0), (404, 0)),
    ((0, 1, 256, 2048, 440, None, 0), (308, 0), (408, 0)), ((0, 1, 256, 2048, 440, "fwd", 0), (304, 0), (404, 0)),
    ((1, 0, 2048, 2048, 256, None, 0), (328, 0), (408, 0)), ((0, 0, 256, 2048, 3000, None, 0), (304, 0), (404, 0)),
    # LC-BLSTM batched products (1920 rows): K split over workgroups where 64 x 128 tiles cannot fill the chip
    ((0, 1, 1920, 2048, 512, None, 0), (351, 0), (408, 0)), ((0, 1, 1920, 2048, 512, "fwd", 0), (308, 0), (408, 0)),
    ((0, 0, 1920, 512, 2048, None, 0), (308, 2), (408, 2)), ((0, 0, 1920, 512, 2048, "indiff", 0), (308, 2), (408, 2)),
    ((1, 0, 2048, 512, 1920, None, 0), (308, 2), (408, 2)), ((1, 0, 2048, 512, 1920, "wgrad", 0), (308, 0), (408, 0)),
    # large squares: 128 x 128 with producer / consumer waves; one plane from two full rounds on
    ((0, 1, 2048, 2048, 2048, None, 0), (351, 0), (408, 0)), ((0, 1, 4096, 2048, 2048, None, 0), (351, 0), (411, 0)),
    ((0, 1, 4096, 4096, 4096, None, 0), (351, 0), (411, 0)), ((1, 0, 4096, 4096, 4096, None, 0), (328, 0), (408, 0)),
    ((0, 1, 4096, 2048, 2048, "fwd", 0), (308, 0), (408, 0)), ((0, 1, 1920, 3000, 1024, None, 0), (308, 0), (408, 0)),
    # ragged
    ((0, 0, 132, 260, 68, None, 0), (308, 0), (408, 0)), ((1, 0, 436, 128, 2052, None, 0), (304, 0), (404, 0)),
    ((0, 1, 192, 1920, 1028, None, 0), (304, 0), (404, 0)), ((1, 1, 512, 640, 768, None, 0), (308, 0), (408, 0)),
    # a tile asked for by number (either plane mode's)
    ((0, 1, 1024, 2048, 2048, None, 304), (304, 0), (404, 0)), ((0, 1, 1024, 2048, 2048, None, 311), (351, 0), (411, 0)),
    ((0, 1, 1024, 2048, 2048, None, 312), (311, 0), (411, 0)), ((0, 1, 1024, 2048, 2048, None, 351), (351, 0), (411, 0)),
    ((0, 1, 1024, 2048, 2048, "fwd", 351), (308, 0), (408, 0)), ((0, 1, 1024, 2048, 2048, None, 328), (0, 0), (408, 0)),
    ((0, 0, 1024, 2048, 2048, None, 311), (308, 0), (408, 0)), ((1, 0, 2048, 2048, 1024, None, 308), (308, 0), (408, 0)),
    ((1, 0, 436, 128, 2052, None, 328), (308, 0), (408, 0)), ((1, 0, 436, 128, 2052, None, 308), (308, 7), (408, 7)),
    ((0, 1, 192, 1920, 1028, None, 308), (308, 4), (408, 4)), ((0, 1, 4096, 4096, 4096, None, 408), (0, 0), (408, 0)),
    # not served
    ((0, 1, 64, 2048, 2048, None, 0), (0, 0), (0, 0)), ((0, 1, 1024, 2048, 2050, None, 0), (0, 0), (0, 0)),
]


def test_library_exports_and_binding(aslp):
    fn = aslp.lib.aslp_gemm_split16_plan
    assert fn.restype is C.c_int and len(fn.argtypes) == 11


@pytest.mark.parametrize("case,two,one", TABLE)
def test_plan_table(aslp, case, two, one):
    tA, tB, M, N, K, kind, cfg = case
    ep = epilogue(aslp, kind, N)
    for planes, want in ((2, two), (1, one)):
        split = C.c_int(-1)
        tile = aslp.lib.aslp_gemm_split16_plan(tA, tB, M, N, K, N, C.byref(ep) if ep is not None else None, None, planes, cfg, C.byref(split))
        assert (tile, split.value) == want, (case, planes)


def test_a_tile_by_its_one_plane_number_and_a_pair(aslp):
    plan = aslp.lib.aslp_gemm_split16_plan
    assert plan(0, 1, 1024, 2048, 2048, 2048, None, None, 1, 404, None) == 404
    assert plan(0, 1, 1024, 2048, 2048, 2048, None, None, 1, 304, None) == 404
    # the two directions of a BLSTM layer in one launch: 2 x 240 tiles of 128 x 128 fill the chip where one product's would not
    E = aslp._lib.GemmEpilogue
    assert plan(0, 1, 1920, 2048, 512, 2048, None, C.byref(E()), 2, 0, None) == 351
    assert plan(0, 1, 1920, 2048, 512, 2048, None, C.byref(E()), 1, 0, None) == 408
    # an epilogue the 16-byte path cannot serve (N % 4 aside, a misaligned bias) loses its planes / maxima request, not the product
    ep = epilogue(aslp, "fwd", 2048)
    ep.bias = A16 + 4
    assert plan(0, 1, 256, 2048, 440, 2048, C.byref(ep), None, 2, 0, None) == 308
