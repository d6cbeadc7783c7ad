"""The one switch for fp16 operands (aslp_fp16_operands / ASLP_FP16_OPERANDS=1, include/aslp_kernels.h) without a device: it changes the
DEFAULT of the per-site switches and nothing else.  A site asks its own setter, then its own environment variable (a value it accepts),
then the umbrella, then its old default.  Checked on the five getters, which launch nothing, in fresh processes that only load the library
(no torch, no GPU) -- one per environment, since every variable is read once per process.

Under the umbrella: layer products one plane, persistent LSTM recurrences one piece, per-timestep LSTM path on, per-timestep GRU path one
piece (it measured faster); the persistent GRU recurrences stay on the fp32 instruction (their fp16 form measured slower)."""
import json
import os
import subprocess
import sys

import pytest

GETTERS = ("aslp_gemm_operand_planes_get", "aslp_lstm_operand_pieces_get", "aslp_lstm_step_split16_get", "aslp_gru_seq_pieces_get",
           "aslp_gru_step_pieces_get")
OFF = [2, 2, 0, 0, 0]        # gemm planes, lstm pieces, lstm step switch, gru seq pieces, gru step pieces
ON = [1, 1, 1, 0, 1]
VARIABLES = ("ASLP_FP16_OPERANDS", "ASLP_GEMM_PLANES", "ASLP_LSTM_PIECES", "ASLP_LSTM_STEP_SPLIT_F16", "ASLP_GRU_SEQ_PIECES", "ASLP_GRU_STEP_PIECES")

CHILD = r'''
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1], mode=ctypes.RTLD_GLOBAL)
out = []
for call in json.loads(sys.argv[2]):
    if call == "get":
        out.append([int(getattr(lib, g)()) for g in %r] + [int(lib.aslp_fp16_operands_get())])
    else:
        getattr(lib, call[0])(int(call[1]))
print(json.dumps(out))
''' % (GETTERS,)


@pytest.fixture
def child(aslp):
    """child(calls, **env): the getters' values (and the umbrella's) at every "get" of `calls`, in a fresh process under `env`"""
    return lambda calls, **env: run_child(aslp._lib.LIB_PATH, calls, env)


def run_child(lib_path, calls, env):
    full = {k: v for k, v in os.environ.items() if k not in VARIABLES}
    full.update(env)
    p = subprocess.run([sys.executable, "-c", CHILD, lib_path, json.dumps(calls)], env=full, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    return json.loads(p.stdout.decode())


def test_nothing_set(child):
    assert child(["get"]) == [OFF + [0]]


@pytest.mark.parametrize("value,on", [("1", True), ("0", False), ("", False), ("2", False), ("10", False), ("yes", False)])
def test_umbrella_by_environment(child, value, on):
    """only "1" turns it on"""
    assert child(["get"], ASLP_FP16_OPERANDS=value) == [(ON if on else OFF) + [int(on)]]


def test_umbrella_by_setter_and_back(child):
    got = child([["aslp_fp16_operands", 1], "get", ["aslp_fp16_operands", 0], "get", ["aslp_fp16_operands", 1], "get", ["aslp_fp16_operands", -1], "get"])
    assert got == [ON + [1], OFF + [0], ON + [1], OFF + [0]]
    # -1 hands the choice back to the variable, 0 beats it
    got = child(["get", ["aslp_fp16_operands", 0], "get", ["aslp_fp16_operands", -1], "get"], ASLP_FP16_OPERANDS="1")
    assert got == [ON + [1], OFF + [0], ON + [1]]


@pytest.mark.parametrize("name,value,site,want", [("ASLP_GEMM_PLANES", "2", 0, 2), ("ASLP_LSTM_PIECES", "2", 1, 2), ("ASLP_LSTM_STEP_SPLIT_F16", "0", 2, 0),
                                                  ("ASLP_GRU_STEP_PIECES", "0", 4, 0), ("ASLP_GRU_STEP_PIECES", "2", 4, 2), ("ASLP_GRU_SEQ_PIECES", "1", 3, 1),
                                                  ("ASLP_GEMM_PLANES", "1", 0, 1)])
def test_a_sites_own_variable_beats_the_umbrella(child, name, value, site, want):
    expect = list(ON)
    expect[site] = want
    assert child(["get"], ASLP_FP16_OPERANDS="1", **{name: value}) == [expect + [1]]
    # ... and means what it meant without the umbrella
    expect = list(OFF)
    expect[site] = want
    assert child(["get"], **{name: value}) == [expect + [0]]


@pytest.mark.parametrize("name,value", [("ASLP_GEMM_PLANES", "7"), ("ASLP_LSTM_PIECES", "x"), ("ASLP_LSTM_STEP_SPLIT_F16", "10"), ("ASLP_GRU_STEP_PIECES", "3")])
def test_a_value_the_site_does_not_accept_is_no_choice(child, name, value):
    assert child(["get"], ASLP_FP16_OPERANDS="1", **{name: value}) == [ON + [1]]
    assert child(["get"], **{name: value}) == [OFF + [0]]


@pytest.mark.parametrize("setter,value,site", [("aslp_gemm_operand_planes", 2, 0), ("aslp_lstm_operand_pieces", 2, 1), ("aslp_lstm_step_split16", 0, 2),
                                               ("aslp_gru_seq_pieces", 2, 3), ("aslp_gru_step_pieces", 2, 4), ("aslp_gru_step_pieces", 0, 4)])
def test_a_sites_setter_beats_the_umbrella_and_its_variable(child, setter, value, site):
    expect = list(ON)
    expect[site] = value
    got = child([[setter, value], "get", [setter, -1], "get"], ASLP_FP16_OPERANDS="1")
    assert got == [expect + [1], ON + [1]]                  # -1: back to the umbrella's default
    # the setter first, the site's variable second, the umbrella third
    own = {"aslp_gemm_operand_planes": ("ASLP_GEMM_PLANES", "1", 1), "aslp_lstm_operand_pieces": ("ASLP_LSTM_PIECES", "1", 1),
           "aslp_lstm_step_split16": ("ASLP_LSTM_STEP_SPLIT_F16", "1", 1), "aslp_gru_seq_pieces": ("ASLP_GRU_SEQ_PIECES", "1", 1),
           "aslp_gru_step_pieces": ("ASLP_GRU_STEP_PIECES", "1", 1)}[setter]
    by_variable = list(ON)
    by_variable[site] = own[2]
    got = child([[setter, value], "get", [setter, -1], "get", ["aslp_fp16_operands", 0], "get"], ASLP_FP16_OPERANDS="1", **{own[0]: own[1]})
    off_by_variable = list(OFF)
    off_by_variable[site] = own[2]
    assert got == [expect + [1], by_variable + [1], off_by_variable + [0]]


def test_the_split_switches_still_win_where_they_did(child):
    """ASLP_GEMM_SPLIT_F16=0 / ASLP_LSTM_SPLIT_F16=0 put their products on the fp32 instruction whatever the piece counts say; the umbrella
    moves neither switch (their state has no getter: the C ABI's plan and probe calls show it on the GPU) and the counts read as under it"""
    assert child(["get"], ASLP_FP16_OPERANDS="1", ASLP_GEMM_SPLIT_F16="0", ASLP_LSTM_SPLIT_F16="0") == [ON + [1]]


def test_context_manager_restores(aslp):
    lib, ops = aslp.lib, aslp.ops
    sites = lambda: [int(getattr(lib, g)()) for g in GETTERS]
    ops.set_fp16_operands(-1)
    assert lib.aslp_fp16_operands_get() == 0 and sites() == OFF, "the suite runs with ASLP_FP16_OPERANDS and the sites' variables unset"
    try:
        with ops.fp16_operands(1):
            assert lib.aslp_fp16_operands_get() == 1 and sites() == ON
            with ops.fp16_operands(0):
                assert lib.aslp_fp16_operands_get() == 0 and sites() == OFF
            assert lib.aslp_fp16_operands_get() == 1 and sites() == ON
            with ops.gru_step_pieces(2), ops.operand_planes(2):       # a site's own setting inside the block wins
                assert sites() == [2, 1, 1, 0, 2]
            ops.set_gru_step_pieces(-1)
            ops.set_operand_planes(-1)
            assert sites() == ON
        assert lib.aslp_fp16_operands_get() == 0 and sites() == OFF
        with pytest.raises(ZeroDivisionError):
            with ops.fp16_operands(1):
                1 / 0
        assert lib.aslp_fp16_operands_get() == 0 and sites() == OFF    # restored although the body raised
        ops.set_fp16_operands(1)
        assert sites() == ON
        ops.set_fp16_operands(-1)
        assert sites() == OFF
    finally:
        ops.set_fp16_operands(-1)
        ops.set_gru_step_pieces(-1)
        ops.set_operand_planes(-1)
