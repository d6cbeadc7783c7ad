"""The float64 models of tests/temporal_ref.py pinned against the oracle (oracle/aslp_oracle_temporal.c, fp32), on every case of the tables of
tests/test_temporal_kernels_gpu.py: the oracle lies within the DERIVED bars element by element on every output of two consecutive calls, its
zeros past a stream's length are exact, its clip follows the exact rule -- so the bars are ones the reference alone keeps -- and the tables
meet the conditions the GPU file relies on (every path of the host rules, the clip classes, ragged lengths).  Needs no GPU."""
import numpy as np
import pytest

import temporal_ref as ref

ratios = {}   # group -> largest err / bar of the oracle


def note(group, r):
    ratios[group] = max(ratios.get(group, 0.0), r)


def rc_oracle_calls(oracle, inp):
    """the two calls by the oracle, on the streams that are not empty (an empty stream makes it read the row before the matrix); yields
    (k, state before, outputs, the rows of those streams)"""
    c = inp.case
    live = np.flatnonzero(inp.lens > 0)
    rows = (np.arange(c.T)[:, None] * c.S + live[None, :]).ravel()
    m = oracle.RowConv(c.D, c.K, np.random.default_rng(0))
    m.w[:], m.w_corr[:] = inp.w, inp.w_corr
    for k in range(2):
        before = m.w.copy(), m.w_corr.copy()
        out = m.propagate(inp.x[k][rows], c.T, len(live), inp.lens[live])
        idf = m.backpropagate(inp.od[k][rows], c.T, len(live), inp.lens[live])
        m.update(ref.LR, ref.MMT)
        yield k, before, dict(out=out, in_diff=idf, w_diff=m.w_diff.copy(), w_corr=m.w_corr.copy(), w=m.w.copy()), rows


@pytest.mark.parametrize("name", ref.RC_NAMES)
def test_rowconv_oracle_within_the_bars(oracle, name):
    inp = ref.rc_inputs(ref.RC_BY_NAME[name])
    c, fails = inp.case, []
    for k, (w0, c0), got, rows in rc_oracle_calls(oracle, inp):
        want = ref.rowconv_model(w0, c0, inp.x[k], inp.od[k], c.T, c.S, inp.lens)
        for key in ("out", "in_diff"):
            sub = ref.Out(*(a[rows] for a in want[key]))
            note("rowconv " + key, ref.check(got[key], sub, "%s call %d %s" % (name, k, key), fails))
            past = (np.arange(c.T)[:, None] >= inp.lens[None, :]).ravel()   # rows t * S + s with t >= L_s
            assert not want[key].v[past].any() and not want[key].bar[past].any(), (name, key, "the model past the length")
            assert not got[key][past[rows]].any(), (name, key, "the oracle past the length")
        for key in ("w_diff", "w_corr", "w"):
            note("rowconv " + key, ref.check(got[key], want[key], "%s call %d %s" % (name, k, key), fails))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", ref.FSMN_NAMES)
def test_fsmn_oracle_within_the_bars(oracle, name):
    inp = ref.fsmn_inputs(ref.FSMN_BY_NAME[name])
    c, fails = inp.case, []
    m = oracle.Fsmn(c.D, c.P, c.F, np.random.default_rng(0))
    m.coef[:] = inp.coef
    for k in range(2):
        want = ref.fsmn_model(m.coef, inp.x[k], inp.od[k], c.P, c.F, inp.clip[k])
        out = m.propagate(inp.x[k])
        idf = m.backpropagate(inp.x[k], inp.od[k], inp.clip[k])
        corr = m.corr.copy()
        m.update(ref.LR)
        for key, got in (("out", out), ("in_diff", idf), ("corr", corr), ("coef", m.coef)):
            note("fsmn " + key, ref.check(got, want[key], "%s call %d %s" % (name, k, key), fails))
        if c.clip:
            assert inp.clip[k] > 0.0
            ref.check_clip(corr, want, inp.clip[k], "%s call %d corr" % (name, k), fails)
            n = want["sure"].size
            clipped, either = np.count_nonzero(want["sure"]), np.count_nonzero(want["either"])
            assert either <= 0.01 * n and clipped >= 0.25 * n and n - clipped - either >= 0.25 * n, (name, k, n, clipped, either)
    assert not fails, "\n".join(fails)


def test_rowconv_table_reaches_every_path():
    """the conditions the GPU file relies on, by the host rules as temporal_ref restates them"""
    cases = ref.RC_CASES
    fwd = {(c.K, ref.rc_paths(c)[0]) for c in cases}
    bwd = {(c.K, ref.rc_paths(c)[1]) for c in cases}
    ring = {0: 4, 2: 4, 3: 4, 4: 8, 7: 8, 8: 16, 15: 16, 20: 21, 16: 32, 19: 32, 21: 32, 31: 32}
    for K, r in ring.items():
        assert ref.rc_ring(K) == r and (K, r) in fwd and (K, r) in bwd, (K, r)
    assert all(ref.rc_ring(K) == 0 and (K, 0) in fwd and (K, 0) in bwd for K in (32, 63, 64))
    plain = [c for c in cases if ref.rc_paths(c)[1] == 0 and c.K < 32]
    assert any(c.D % 2 for c in plain) and {c.odd for c in plain if c.D % 2 == 0} >= {"x", "od", "y"} and any(c.offset for c in plain)
    assert ref.rc_paths(ref.RC_BY_NAME["odd-ld-out-diff"]) == (8, 0)      # the forward does not see out_diff
    assert {c.D for c in cases} >= {2, 126, 128, 130} and {c.S for c in cases} >= {1, 4, 5, 20} and {c.T for c in cases} >= {1, 60, 63, 64, 65, 130}
    strips = lambda c: -(-c.D // ref.RC_COLS) * -(-c.S // ref.RC_STREAMS)
    assert any(strips(c) == 10 for c in cases)
    for c in cases:
        lens = set(c.lens)
        assert c.one_sided or (c.T in lens and any(l < c.T for l in lens)), c.name
    lens = {(l, c.T) for c in cases for l in c.lens}
    assert any(l == 1 for l, T in lens) and any(l == 64 for l, T in lens) and any(l == 65 for l, T in lens) and any(l == T - 1 for l, T in lens)
    assert any(l == 0 for l, T in lens)
    # an L with L + K one row into the next chunk of the backward, and one on the edge; more backward chunks than forward chunks
    edge = [(c, l) for c in cases if ref.rc_paths(c)[1] for l in c.lens if l > 0]
    assert any((l + c.K) % ref.RC_CHUNK == 1 for c, l in edge) and any((l + c.K) % ref.RC_CHUNK == 0 for c, l in edge)
    assert any(ref.rc_paths(c)[1] and -(-(c.T + c.K) // ref.RC_CHUNK) > -(-c.T // ref.RC_CHUNK) for c in cases)
    # a workgroup with one stream inside S
    assert any(ref.rc_paths(c)[1] and c.S % ref.RC_STREAMS == 1 and c.S > 1 for c in cases)


def test_fsmn_table_reaches_every_path():
    cases = ref.FSMN_CASES
    Cs = {c.P + c.F + 1 for c in cases}
    assert Cs >= {1, 6, 7, 8, 9, 64, 65, 73, 74, 126, 127, 216, 217}
    assert [ref.fsmn_paths(ref.FsmnCase("", 1, C - 1, 0, 1, False)) for C in (126, 127, 216, 217)] == [(True, True), (True, False), (True, False), (False, False)]
    assert {ref.fsmn_paths(c) for c in cases} == {(True, True), (True, False), (False, False)}
    assert any(c.P == 0 and c.F == 0 for c in cases) and any(c.P == 0 and c.F > 0 for c in cases) and any(c.P > 0 and c.F == 0 for c in cases)
    assert {c.D for c in cases} >= {1, 63, 64, 65} and {c.T for c in cases} >= {1, 31, 32, 33, 1024, 1025, 2081} and any(c.T < c.P for c in cases)
    assert {-(-c.T // ref.FSMN_FRAMES) for c in cases if ref.fsmn_paths(c)[1]} >= {32, 33, 66}
    assert {ref.fsmn_paths(c)[1] for c in cases if c.clip} == {True, False}
    assert {c.P + c.F + 1 for c in cases if c.clip} == {61, 130}


def test_the_oracles_ratios():
    """runs last: how much of each bar the oracle uses (for information; a ratio above 1 has failed above)"""
    for g, r in sorted(ratios.items()):
        print("    %-18s %.3f" % (g, r))
    assert all(r <= 1.0 for r in ratios.values())
