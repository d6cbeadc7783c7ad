"""The switch for split-fp16 layer products at sizes that are no multiple of 4 (ASLP_GEMM_S16_RAGGED / aslp_gemm_split16_ragged,
csrc/gemm_split16.hip) without a device: who decides -- setter > environment > default off -- and what aslp_gemm_split16_plan, which
launches nothing, answers for ragged shapes with the switch off and on."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO_PLANE_TILES = (304, 308, 311, 328, 351)
ONE_PLANE_TILES = (404, 408, 411)


@pytest.fixture(autouse=True)
def switch_back_afterwards(aslp):
    yield
    aslp.lib.aslp_gemm_split16_ragged(-1)
    aslp.lib.aslp_gemm_split16(-1)


def fresh(code, **env_changes):
    """`code` with `aslp` loaded in a new process; the environment is this one's without the switch, plus env_changes"""
    env = {k: v for k, v in os.environ.items() if k != "ASLP_GEMM_S16_RAGGED"}
    env.update(env_changes)
    head = "import sys\nsys.path.insert(0, %r)\nimport aslp_import\naslp = aslp_import.load()\nget = aslp.lib.aslp_gemm_split16_ragged_get\n" % ROOT
    r = subprocess.run([sys.executable, "-c", head + code + "\nprint('ragged-ok')\n"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ragged-ok" in r.stdout, (r.returncode, r.stdout[-400:], r.stderr[-800:])


def test_default_is_off():
    fresh("assert get() == 0\n"
          "aslp.lib.aslp_gemm_split16_ragged(1); assert get() == 1\n"
          "aslp.lib.aslp_gemm_split16_ragged(0); assert get() == 0\n"
          "aslp.lib.aslp_gemm_split16_ragged(-1); assert get() == 0")


@pytest.mark.parametrize("value,on", [("1", 1), ("0", 0), ("2", 0), ("", 0), ("10", 0), ("yes", 0)])
def test_only_1_in_the_environment_turns_it_on(value, on):
    fresh("assert get() == %d" % on, ASLP_GEMM_S16_RAGGED=value)


def test_the_setter_wins_over_the_environment_and_hands_back():
    fresh("assert get() == 1\n"
          "aslp.lib.aslp_gemm_split16_ragged(0); assert get() == 0\n"
          "aslp.lib.aslp_gemm_split16_ragged(-1); assert get() == 1\n"
          "with aslp.ops.split16_ragged(0):\n    assert get() == 0\n"
          "assert get() == 1", ASLP_GEMM_S16_RAGGED="1")
    fresh("aslp.ops.set_split16_ragged(1); assert get() == 1\n"
          "with aslp.ops.split16_ragged(0):\n    assert get() == 0\n"
          "assert get() == 1\n"
          "aslp.ops.set_split16_ragged(-1); assert get() == 0", ASLP_GEMM_S16_RAGGED="0")


def test_independent_of_the_other_switches():
    """no member of the fp16-operands umbrella, untouched by the plane count; ASLP_GEMM_SPLIT_F16=0 still refuses everything"""
    fresh("assert get() == 0 and aslp.lib.aslp_gemm_operand_planes_get() == 1", ASLP_FP16_OPERANDS="1")
    fresh("assert get() == 1 and aslp.lib.aslp_gemm_operand_planes_get() == 2\n"
          "assert aslp.lib.aslp_gemm_split16_plan(0, 1, 129, 131, 67, 131, None, None, 2, 0, None) in (304, 308, 311, 351)", ASLP_GEMM_S16_RAGGED="1")
    fresh("assert get() == 1\n"
          "assert aslp.lib.aslp_gemm_split16_plan(0, 1, 129, 131, 67, 131, None, None, 2, 0, None) == 0\n"
          "assert aslp.lib.aslp_gemm_split16_plan(0, 1, 1024, 2048, 2048, 2048, None, None, 2, 0, None) == 0",
          ASLP_GEMM_S16_RAGGED="1", ASLP_GEMM_SPLIT_F16="0")


@pytest.mark.parametrize("tA,tB", [(0, 1), (0, 0), (1, 0), (1, 1)])
def test_plan_of_a_ragged_shape(aslp, tA, tB):
    plan = aslp.lib.aslp_gemm_split16_plan
    for planes, tiles in ((2, TWO_PLANE_TILES), (1, ONE_PLANE_TILES)):
        aslp.lib.aslp_gemm_split16_ragged(0)
        assert plan(tA, tB, 129, 131, 67, 131, None, None, planes, 0, None) == 0
        aslp.lib.aslp_gemm_split16_ragged(1)
        assert plan(tA, tB, 129, 131, 67, 131, None, None, planes, 0, None) in tiles
        # one extent ragged at a time, and the three floors, which stay
        for M, N, K in ((131, 128, 64), (128, 131, 64), (128, 128, 67)):
            assert plan(tA, tB, M, N, K, N, None, None, planes, 0, None) in tiles, (M, N, K)
        for M, N, K in ((127, 131, 67), (129, 127, 67), (129, 131, 63)):
            assert plan(tA, tB, M, N, K, N, None, None, planes, 0, None) == 0, (M, N, K)
        with aslp.ops.split16_ragged(0):
            assert plan(tA, tB, 129, 131, 67, 131, None, None, planes, 0, None) == 0
        assert aslp.lib.aslp_gemm_split16_ragged_get() == 1


# (the three TN shapes that are multiples of 4 and not of 8, on grids where the 128 x 128 kernel for two reduction-major operands would be
# chosen if they were multiples of 8: they stay on 64 x 128 with the switch on as with it off; asked for by number, 328 is refused alike)
@pytest.mark.parametrize("shape", [(0, 0, 132, 260, 68), (0, 1, 1000, 3000, 440), (1, 0, 2048, 2048, 1024), (0, 1, 256, 2048, 2048), (0, 0, 1920, 512, 2048),
                                   (0, 1, 64, 2048, 2048), (1, 0, 4100, 2048, 1024), (1, 0, 2052, 4096, 1024), (1, 0, 4100, 4100, 512),
                                   (1, 0, 4096, 2052, 1024)])
def test_a_multiple_of_4_gets_the_same_answer_either_way(aslp, shape):
    import ctypes as C
    tA, tB, M, N, K = shape
    for planes in (2, 1):
        for cfg in (0, 328, 308, 304):
            got = []
            for on in (0, 1):
                aslp.lib.aslp_gemm_split16_ragged(on)
                split = C.c_int(-1)
                got.append((aslp.lib.aslp_gemm_split16_plan(tA, tB, M, N, K, N, None, None, planes, cfg, C.byref(split)), split.value))
            assert got[0] == got[1], (shape, planes, cfg, got)
            if planes == 2 and cfg in (0, 328) and tA and not tB and M >= 2048 and (M % 8 or N % 8):
                assert got[0][0] == 308, (shape, cfg, got)


def test_the_128_x_128_kernel_for_two_reduction_major_operands(aslp):
    """gemm_s16_ks128 (328) asks for M and N multiples of 8 among the multiples of 4; an M or N that is no multiple of 4 -- served under the
    switch only -- is taken where its multiple-of-8 neighbour is: the weight gradient of a 4101-pdf output layer, and by number"""
    plan = aslp.lib.aslp_gemm_split16_plan
    aslp.lib.aslp_gemm_split16_ragged(1)
    assert plan(1, 0, 4104, 2048, 1024, 2048, None, None, 2, 0, None) == 328
    assert plan(1, 0, 4101, 2048, 1024, 2048, None, None, 2, 0, None) == 328
    assert plan(1, 0, 4096, 2049, 1024, 2052, None, None, 2, 0, None) == 328
    assert plan(1, 0, 4100, 2048, 1024, 2048, None, None, 2, 0, None) == 308
    assert plan(1, 0, 259, 261, 131, 264, None, None, 2, 328, None) == 328 and plan(1, 0, 260, 264, 131, 264, None, None, 2, 328, None) == 308
    assert plan(1, 0, 4101, 2048, 1024, 2048, None, None, 1, 0, None) == 408        # (no one-plane form)
    aslp.lib.aslp_gemm_split16_ragged(0)
    assert plan(1, 0, 4101, 2048, 1024, 2048, None, None, 2, 0, None) == 0


def test_a_ragged_shape_whose_reduction_is_split(aslp):
    """the two shapes tests/test_gemm_ragged_gpu.py runs: 1001 x 515 x 2051 -- 80 tiles of 64 x 128 cannot fill the chip, more than 256 of
    32 x 64, a long K: chunks of K over workgroups by the heuristic -- and 130 x 131 x 2051 with the 64 x 128 tile asked for by number (left
    alone it runs whole on 15 tiles of 32 x 64); each as its multiple-of-4 neighbour"""
    import ctypes as C
    aslp.lib.aslp_gemm_split16_ragged(1)
    for planes, tile in ((2, 308), (1, 408)):
        for tA, tB in ((0, 1), (0, 0), (1, 0)):
            for (M, N, K), (M4, N4, K4), cfg in (((1001, 515, 2051), (1004, 516, 2052), 0), ((130, 131, 2051), (132, 132, 2052), 308)):
                split, split4 = C.c_int(-1), C.c_int(-1)
                assert aslp.lib.aslp_gemm_split16_plan(tA, tB, M, N, K, N, None, None, planes, cfg, C.byref(split)) == tile
                assert aslp.lib.aslp_gemm_split16_plan(tA, tB, M4, N4, K4, N4, None, None, planes, cfg, C.byref(split4)) == tile
                assert split.value >= 2 and split.value == split4.value, (planes, tA, tB, M, split.value, split4.value)
    aslp.lib.aslp_gemm_split16_ragged(0)
    assert aslp.lib.aslp_gemm_split16_plan(0, 1, 1001, 515, 2051, 515, None, None, 2, 0, None) == 0
