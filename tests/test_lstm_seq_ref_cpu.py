"""CPU-only: what tests/test_lstm_seq_kernels_gpu.py stands on.
  * the float64 model of the aslp_lstm_seq contract (tests/lstm_seq_ref.py) is pinned to the oracle (oracle/aslp_oracle_rnn.c);
  * the case list, taken over the switches and the child processes' settings, launches every one of the 36 persistent LSTM kernels -- counted
    from the dispatch ladders restated here, no kernel names or compiler output involved;
  * the cases' inputs are benign: the same model in float32 stays within the GPU tests' bar of the float64 run, so a GPU comparison that
    fails cannot be blamed on saturated gates or a chaotic recurrence."""
import ctypes as C
import importlib.util
import itertools
import os
import subprocess

import numpy as np
import pytest

import lstm_seq_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the model against the oracle ------------------------------------------------------------------------------------------------------

def oracle_case(p, x, od, T, S, reverse, lens, state):
    """One direction of an oracle component as a model input: the x-part + bias and dL/dm formed in float64, W_eff = W_r W_rm in float64;
    with a projection and a carried state the first step's recurrent term is r(0) W_r^T, r(0) from the history's r columns."""
    G, Cc, R = 3 if p.cifg else 4, p.C, p.R
    W = (G + 3) * Cc
    first = R > 0 and state is not None
    c = ref.Case(Cc, S, T, 1, p.cifg, 0, R if first else 0, W if first else 0, 0, 1, 0, ())
    f64 = lambda a: np.asarray(a, np.float64)
    y = np.zeros((T + 2, S, p.width))
    y[1:T + 1, :, :G * Cc] = (f64(x) @ f64(p.w_x).T + f64(p.bias)).reshape(T, S, G * Cc)
    if state is not None:
        y[T + 1 if reverse else 0] = state
    w_eff = f64(p.w_r) @ f64(p.w_rm) if R > 0 else f64(p.w_r)
    d = np.zeros((T + 2, S, p.width))
    d[1:T + 1, :, (G + 2) * Cc:W] = (f64(od) @ f64(p.w_rm) if R > 0 else f64(od)).reshape(T, S, Cc)
    q = dict(y=y, d=d, w=w_eff, w_first=f64(p.w_r), peep_i=p.peep_i, peep_f=p.peep_f, peep_o=p.peep_o, reverse=int(reverse))
    return dict(case=c, dirs=[q], lens=lens)


@pytest.mark.parametrize("marker,R,cifg,bidir", [("<Lstm>", 0, 0, 0), ("<BLstm>", 0, 0, 1), ("<LstmCifgProjectedStreams>", 12, 1, 0)])
def test_model_matches_oracle(oracle, marker, R, cifg, bidir):
    """Two batches at C = 20, T = 6, S = 5; the unidirectional members carry their state into the second, <BLstm> masks its backward-in-time
    direction with ragged sequence lengths (0, 1, T - 1 and T among them).  The oracle's fp32 buffers against the float64 model: every
    activation and diff tensor within the bar of the GPU tests."""
    D, Cc, T, S = 7, 20, 6, 5
    rng = np.random.default_rng(3)
    G = 3 if cifg else 4
    W = (G + 3) * Cc
    for reverse in range(2 if bidir else 1):
        p = oracle.LstmDir(D, Cc, R, cifg, rng, scale=0.3)
        state = None
        for batch in range(2):
            x = rng.standard_normal((T * S, D)).astype(np.float32)
            od = rng.standard_normal((T * S, p.rec)).astype(np.float32)
            lens = np.asarray([T, 0, 1, T - 1, 3], np.int32) if (bidir and reverse) else None
            buf = p.forward(x, T, S, reverse=bool(reverse), init_state=state, seq_len=lens)
            dbuf, _ = p.backward(od, T, S, buf, reverse=bool(reverse))
            inp = oracle_case(p, x, od, T, S, reverse, lens, state)
            y = ref.forward(inp, 0)
            d = ref.backward(inp, 0, y)
            got_y, got_d = buf.reshape(T + 2, S, -1), dbuf.reshape(T + 2, S, -1)
            for backward_pass, g, r in ((0, got_y, y), (1, got_d, d)):
                for name, off in ref.tensors(inp["case"], backward_pass) + ([("d_m", (G + 2) * Cc)] if backward_pass else []):
                    l2, el = ref.errors(g[1:T + 1, :, off:off + Cc], r[1:T + 1, :, off:off + Cc])
                    assert l2 < ref.BAR and el < 10 * ref.BAR, (marker, "direction", reverse, "batch", batch, name, l2, el)
            if lens is not None:
                assert not y[1:, 1].any() and not y[2:T + 1, 2].any() and y[1, 2].any() and not y[T, 3].any() and y[T - 1, 3].any()
            if not bidir:
                state = buf.reshape(T + 2, S, -1)[T].copy()   # carried into the second batch: c, h, m (and r) of the last frame


def test_first_step_exceptions_and_windows_of_the_model():
    """skip_first_product leaves the first step's gate pre-activations alone; the r(0) W_first^T term equals the ordinary one when r(0) = m(0)
    and W_first = W_eff; grad_partial chains are counted inside the window and add up to the whole."""
    c = ref.Case(8, 20, 3, 1, 0, 0, 8, 0, 0, 1, 0, ())
    inp = ref.build_case(c)
    q = inp["dirs"][0]
    q["y"][0, :, :8] = q["y"][0, :, 6 * 8:7 * 8]          # r(0) := m(0)
    q["w_first"][:, :8] = q["w"][:, :8]
    plain = dict(inp, case=c._replace(k_first=0))
    assert np.array_equal(ref.forward(inp, 0), ref.forward(plain, 0))
    skipped = dict(inp, case=c._replace(k_first=0, skip=1))
    folded = dict(plain, dirs=[dict(q, y=q["y"].astype(np.float64))])
    folded["dirs"][0]["y"][1, :, :32] += q["y"][0, :, 48:56].astype(np.float64) @ q["w"][:, :8].astype(np.float64).T
    assert np.allclose(ref.forward(dict(folded, case=skipped["case"]), 0)[1:], ref.forward(plain, 0)[1:], rtol=0, atol=1e-14)
    y = ref.forward(plain, 0)
    d = ref.backward(plain, 0, y)
    whole = ref.grad_partial(plain, 0, y, d)
    assert sorted(whole) == [0, 1, 2]
    win = ref.grad_partial(plain, 0, y, d, 8, 5)
    assert sorted(win) == [0] and not np.allclose(win[0], whole[1]) and np.allclose(ref.grad_partial(plain, 0, y, d, 8, 8)[0], whole[1])
    assert ref.dmax(plain, d) == np.abs(d[1:4, :, :32]).max()


# ---- the case list covers every instantiation --------------------------------------------------------------------------------------------

# family: (pass, the switches it serves -> pieces template parameter (None: none), cell-count rungs, FAST is a template parameter)
LADDERS = {
    "lstm_seq_fwd": (0, {"split16=0": None}, (128, 512), True),                      # CIFG x KW 16 / 64 x FAST
    "lstm_seq_fwd_h": (0, {"default": 2, "pieces=1": 1}, (256, 512), True),          # CIFG x NCH 1 / 2 x FAST x NP
    "lstm_seq_bwd": (1, {"split16=0": None}, (128, 512), False),                     # CIFG x TPW 1 / 4
    "lstm_seq_bwd_h": (1, {"default": 2, "pieces=1": 1}, (128, 512), False),         # CIFG x TPW 1 / 4 x NP
}
# (label of the process, FAST, the switches every case runs under there)
PROCESSES = [("in process", True, ("default", "split16=0", "pieces=1")), ("ASLP_LSTM_FAST_ACT=0", False, ("default", "split16=0", "pieces=1")),
             ("ASLP_LSTM_WAVE_COLLECT=0 ASLP_LSTM_READ_AHEAD=0", True, ("default", "split16=0"))]


def all_instantiations():
    out = set()
    for family, (_, switches, rungs, by_fast) in LADDERS.items():
        for cifg, rung, np_, fast in itertools.product((0, 1), range(len(rungs)), set(switches.values()), (True, False) if by_fast else (None,)):
            out.add((family, cifg, rung, fast, np_))
    return out


def launched(case, switch, fast):
    """the two instantiations (forward, backward) a case launches under a switch in a process with that FAST setting"""
    out = []
    for family, (_, switches, rungs, by_fast) in LADDERS.items():
        if switch in switches:
            rung = next(k for k, top in enumerate(rungs) if case.C <= top)
            out.append((family, case.cifg, rung, fast if by_fast else None, switches[switch]))
    assert len(out) == 2
    return out


def test_cases_reach_all_36_kernels():
    every = all_instantiations()
    assert len(every) == 36
    assert [s[0] for s in ref.SWITCHES] == ["default", "split16=0", "pieces=1"]
    hit = {}
    for _, fast, switches in PROCESSES:
        for case, switch in itertools.product(ref.CASES, switches):
            for inst in launched(case, switch, fast):
                hit.setdefault(inst, []).append(case)
    missing = sorted(every - set(hit), key=str)
    assert not missing and set(hit) == every, missing
    print("lstm-seq coverage: %d of %d instantiations launched" % (len(hit), len(every)))
    for family in LADDERS:   # whole and partial last workgroup (16 cells each), per family -- and in fact on every rung of every ladder
        for rung in range(2):
            cells = {c.C for inst, cases in hit.items() if inst[0] == family and inst[2] == rung for c in cases}
            assert any(n % 16 == 0 for n in cells) and any(n % 16 for n in cells), (family, rung, sorted(cells))
    for inst, cases in sorted(hit.items(), key=str):
        print("  %-16s cifg %d rung %d fast %-5s pieces %-4s <- C = %s" % (inst + (sorted({c.C for c in cases}),)))


def test_case_list_holds_what_the_issue_of_the_kernels_names():
    cs = ref.CASES
    assert {c.C for c in cs} == {4, 20, 36, 128, 132, 256, 260, 508, 512}
    assert {1, 5, 9} <= {c.S for c in cs} and any(c.S == 32 and c.ndir == 2 for c in cs) and any(c.S == 64 and c.ndir == 1 for c in cs)
    assert {1, 2, 6, 9} <= {c.T for c in cs}
    assert {(c.k_first, c.C) for c in cs if c.k_first} >= {(4, 4), (40, 128), (128, 128), (256, 132)}
    assert any(c.k_first and c.col_first for c in cs) and any(c.k_first and not c.col_first for c in cs)
    assert any(c.skip for c in cs) and any(not c.gp for c in cs) and any(c.dmax for c in cs) and any(c.ragged for c in cs)
    assert ((0, 32), (32, 1)) in {c.windows for c in cs if c.S == 33 and c.ndir == 2} and ((8, 5),) in {c.windows for c in cs if c.S == 20}
    for c in cs:
        assert c.C % 4 == 0 and c.C <= 512 and not (c.skip and c.k_first) and c.col_first + c.k_first <= ref.gates_of(c) * c.C
        assert not c.k_first or (c.k_first % 4 == 0 and c.k_first <= (128 if c.C <= 128 else 256))   # aslp_lstm_seq_first_product_supported_for
        for s_begin, s_count in c.windows:
            assert s_begin + s_count <= c.S and c.ndir * ((s_count + 7) // 8) <= 8
        inp = ref.build_case(c)
        assert inp["ld"] == (ref.gates_of(c) + 3) * c.C + 8 and inp["ldw"] == c.C + 4 and inp["grad_ld"] == c.C + 4 and inp["ldw_first"] > c.k_first
        if c.ragged and c.S >= 4:
            assert {0, 1, c.T - 1, c.T} <= set(int(v) for v in inp["lens"])
    for cifg in (0, 1):   # coupled gates and separate ones on both rungs of every ladder
        assert all(any(c.cifg == cifg and lo < c.C <= hi for c in cs) for lo, hi in ((0, 128), (128, 256), (256, 512)))


# ---- the inputs are benign ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_float32_run_of_the_model_stays_within_the_bar(case):
    inp = ref.build_case(case)
    ys, ds, parts = ref.reference(inp)
    y32, d32, p32 = ref.reference(inp, np.float32)
    assert all(a.dtype == np.float32 for a in y32 + d32)
    worst = ref.compare(inp, ref.as_got(case, y32, d32, p32), ys, ds, parts, ref.BAR)
    gates = np.concatenate([np.abs(y[1:case.T + 1, :, :ref.gates_of(case) * case.C]).ravel() for y in ys])
    assert np.mean(gates > 0.999) < 0.01, "saturated gates"
    print("lstm-seq float32 model vs float64 %s: l2 %.1e, element %.1e" % ((ref.case_id(case),) + worst))


# ---- the binding ------------------------------------------------------------------------------------------------------------------------------

def test_seq_structures_have_the_headers_layout_and_the_sweep_uses_them(aslp, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "aslp_kernels.h"\nint main() { printf("%zu %zu %zu %zu %zu\\n", sizeof(aslp_lstm_seq_dir), '
                   'sizeof(aslp_lstm_seq), offsetof(aslp_lstm_seq, ndir), offsetof(aslp_lstm_seq, grad_partial), offsetof(aslp_lstm_seq, dmax_parts)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(x) for x in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE).stdout.split()]
    from kaldi_aslp_amd import _lib
    assert sizes == [C.sizeof(_lib.SeqDir), C.sizeof(_lib.Seq), _lib.Seq.ndir.offset, _lib.Seq.grad_partial.offset, _lib.Seq.dmax_parts.offset]
    spec = importlib.util.spec_from_file_location("lstm_seq_sweep", os.path.join(ROOT, "devtools", "lstm_seq_sweep.py"))
    sweep = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sweep)
    assert not hasattr(sweep, "Seq") and not hasattr(sweep, "SeqDir") and len(sweep.CASES) == 11 and len(sweep.SWITCHES) == 3
