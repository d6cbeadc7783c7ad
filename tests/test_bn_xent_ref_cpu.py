"""The float64 models of tests/bn_xent_ref.py pinned against the oracle (the fp32 restatement of the reference's CPU path), and the oracle's own
distance to float64 per output -- the bars of tests/test_bn_xent_kernels_gpu.py, which imports bn_oracle_sequence / xent_data from here.

What the oracle does not have is built out of oracle calls: the folded Sigmoid from orc_sigmoid and orc_diff_sigmoid around Bn, the folded
step from Bn.update(lr) behind Bn.backpropagate.  The oracle sums in fp32, so it lies where fp32 lies: within ORACLE_CAP of float64 on every
output, and far closer on most (printed per case)."""
import numpy as np
import pytest

import bn_xent_ref as ref

# what the oracle is held to on every output of every case, per column group (bn_xent_ref.BN_GROUPS), so that MARGIN x its distance stays a
# real bar: the largest element (oracle_lib.max_err) in every group, the relative l2 where the group's reference is not small by cancellation
# (`rest`: a single column's gradient sum, or in_diff at two rows, can be -- there only the element distance is capped).
#   flat     the fp32 mean of rows x 3.25 may lie one ulp (2^-22) off 3.25 where 1 / rows is not exact, and inv_std = 1 / sqrt(floor) = 3162
#            turns that into 7.5e-4 where float64 has an exact zero -- in the reference, the oracle and the kernels alike (all three form
#            fl(fl(sum) fl(1 / rows)) from an exact sum: the same number); the same in every row, a gradient sum over the column carries up to
#            sqrt(rows) times as much: 2.4e-2 at 1024 rows, with a factor 4 for the draw
#   mean100  the fp32 sum of up to 1025 values near 100 carries sqrt(rows) half-ulps of 1e5, 1e-4 of the column's unit deviation in the mean;
#            the error is the same in every row, so a gradient sum over the column carries sqrt(rows) inv_std times as much: 3e-3
#   rest     the project's 1e-4
ORACLE_CAP = {"mean100": 1e-2, "flat": 1e-1, "rest": 1e-4}
_xent = {}


def dist(oracle, a, r):
    return ref.rel_l2(a, r), oracle.max_err(a, r)


def bn_oracle_sequence(oracle, inp, has_y, step):
    """the two calls of bn_xent_ref.bn_sequence by the oracle: same keys, fp32"""
    bn = oracle.Bn(inp.case.cols)
    bn.scale[:], bn.shift[:], bn.dscale[:], bn.dshift[:] = inp.scale, inp.shift, inp.dscale0, inp.dshift0
    calls = []
    for k in range(2):
        out = bn.propagate(inp.x[k])
        o = dict(out=out, xhat=bn.xs.copy(), mean=bn.mean.copy(), inv_std=bn.var.copy(), acc_means=bn.acc_means.copy(), acc_vars=bn.acc_vars.copy())
        dy = inp.od[k]
        if has_y:
            o["act"] = oracle.unary("orc_sigmoid", out)
            dy = oracle.binary("orc_diff_sigmoid", o["act"], inp.od[k])
        o["in_diff"] = bn.backpropagate(inp.x[k], dy, ref.MMT)
        o["D"] = bn.xs.copy()
        if step:
            bn.update(ref.LR)
        o.update(dscale=bn.dscale.copy(), dshift=bn.dshift.copy(), scale=bn.scale.copy(), shift=bn.shift.copy())
        calls.append(o)
    return calls


def bn_distances(oracle, got, want):
    """per call, output and column group: (relative l2, largest element) of `got` to the float64 `want`"""
    return [{k: ref.col_dist(g[k], w[k]) for k in w} for g, w in zip(got, want)]


def xent_oracle(oracle, inp, target, use_softmax):
    y = oracle.unary("orc_softmax_rows", inp.logits) if use_softmax else inp.post
    diff, st = oracle.xent_eval(inp.fw, y, inp.onehot if target != "soft" else inp.soft)
    return diff, y, np.array([st["frames"], st["correct"], st["loss"], st["entropy"], st["likelyhood"]])


def xent_data(oracle, name):
    """inputs of a case and, per (target kind, softmax): the float64 result, the oracle's sums and the oracle's distances on diff and on the
    posteriors.  Computed once per module and shared, never modified.  A label target is the one-hot row of that label."""
    if name not in _xent:
        inp = ref.xent_inputs(ref.XENT_BY_NAME[name])
        res = {}
        for target in ("onehot", "soft"):
            for sm in ((False, True) if ref.softmax_supported(inp.case.cols) else (False,)):
                d64, p64, s64 = ref.xent(inp.logits if sm else inp.post, inp.onehot if target == "onehot" else inp.soft, inp.fw, sm)
                od, op, osum = xent_oracle(oracle, inp, target, sm)
                res[(target, sm)] = dict(diff=d64, post=p64, sums=s64, orc_sums=osum, orc_diff=od, d_diff=dist(oracle, od, d64), d_post=dist(oracle, op, p64))
        _xent[name] = (inp, res)
    return _xent[name]


def test_group_distances_are_rel_l2_and_max_err_of_the_column_slices(oracle):
    rng = np.random.default_rng(1)
    a, r = rng.standard_normal((9, 7)) * 30, rng.standard_normal((9, 7)) * 30
    for g, s in ref.BN_GROUPS:
        assert np.allclose(ref.col_dist(a, r)[g], dist(oracle, a[:, s], r[:, s]), rtol=1e-14, atol=0)
        assert np.allclose(ref.col_dist(a[0], r[0])[g], dist(oracle, a[0, s], r[0, s]), rtol=1e-14, atol=0)


def test_case_tables_name_what_the_host_rule_picks():
    """on 256 CUs; the GPU file asks the library itself (aslp_bn_path)"""
    for c in ref.BN_CASES:
        assert ref.bn_path(c.rows, c.cols) == (("panel", 1, 4) if c.offset else (c.path, c.q, c.slots)), c
    reached = {(c.path, c.q, c.slots) for c in ref.BN_CASES}
    assert {("panel", 1, s) for s in (4, 8, 16)} <= reached and {("coop", q, s) for q, s in ((4, 4), (4, 8), (3, 8), (3, 16), (2, 4), (2, 16))} <= reached
    assert [ref.bn_stats_q(r, c) for r, c in ref.BN_STATS_SHAPES] == [1, 2, 4, 8, 8]
    assert [c.kernel for c in ref.XENT_CASES] == ref.XENT_EXPECT
    assert {"per%d-%s" % (p, m) for p in (4, 8, 16, 32) for m in ("vec", "scalar")} | {"wide"} == set(ref.XENT_EXPECT)
    for c in ref.BN_CASES:   # the kernels and the oracle must be handed the same 1 / rows
        assert np.float32(1.0) / np.float32(c.rows) == np.float32(1.0 / c.rows)


@pytest.mark.parametrize("name", ref.BN_NAMES)
def test_bn_model_matches_oracle(oracle, name):
    inp = ref.bn_inputs(ref.BN_BY_NAME[name])
    cache = {}
    for has_y in (False, True):
        for step in (False, True):
            want = ref.bn_sequence(inp, has_y, step, cache)
            d = bn_distances(oracle, bn_oracle_sequence(oracle, inp, has_y, step), want)
            for k, (dk, w) in enumerate(zip(d, want)):
                for g in ORACLE_CAP:
                    print("bn %-22s y %d step %d call %d %-7s: %s" % (name, has_y, step, k, g, "  ".join("%s %.1e/%.1e" % ((o,) + v[g]) for o, v in dk.items())))
                for o, v in dk.items():
                    for g, cap in ORACLE_CAP.items():
                        if o in ("acc_means", "acc_vars"):
                            assert v[g][0] < 1e-12 * inp.case.rows + 1e-9, (o, g, v[g])
                        else:
                            # (at two rows xhat is +-1 and in_diff cancels to zero: no relative distance)
                            assert (g != "rest" or inp.case.rows <= 2 or v[g][0] < cap) and v[g][1] < cap, (has_y, step, k, o, g, v[g])
                # the column of one value: no variance, inv_std = 1 / sqrt(floor); the zero column: zero out of the normalisation
                assert abs(w["inv_std"][1] - ref.VAR_FLOOR ** -0.5) < 1e-9 and abs(w["inv_std"][2] - ref.VAR_FLOOR ** -0.5) < 1e-9
                assert not w["xhat"][:, 1:3].any()
            if step:   # in_diff is formed with the scale from before the step
                again = ref.bn_backward(inp.x[0], ref.bn_forward(inp.x[0], inp.scale, inp.shift), inp.od[0], inp.scale, inp.dscale0, inp.dshift0, has_y)
                assert np.array_equal(again["in_diff"], want[0]["in_diff"]) and not np.array_equal(want[0]["scale"], inp.scale.astype(np.float64))


@pytest.mark.parametrize("rows,cols", ref.BN_STATS_SHAPES)
def test_bn_stats_shapes_model_matches_oracle(oracle, rows, cols):
    """the forward of the aslp_bn_forward_stats cases (the GPU file takes its bars from the same call)"""
    inp = ref.bn_inputs(ref.BnCase("stats-%dx%d" % (rows, cols), rows, cols, "stats", 0, 0, False), seed=3000 + rows + cols)
    d = bn_distances(oracle, bn_oracle_sequence(oracle, inp, True, False), ref.bn_sequence(inp, True, False))[0]
    for o in ("out", "act", "mean", "inv_std"):
        for g, cap in ORACLE_CAP.items():
            assert (g != "rest" or d[o][g][0] < cap) and d[o][g][1] < cap, (o, g, d[o][g])


@pytest.mark.parametrize("name", ref.XENT_NAMES)
def test_xent_model_matches_oracle(oracle, name):
    inp, res = xent_data(oracle, name)
    c = inp.case
    # the arg-max condition: no row's arg-max hangs on a rounding, so no row is left out of any comparison
    assert (ref.argmax_gap(inp.post) > ref.ARGMAX_GAP).all() and (ref.argmax_gap(ref.softmax(inp.logits)) > ref.ARGMAX_GAP).all()
    assert (inp.labels == -1).sum() >= 1 and (inp.labels == c.cols).sum() >= 1 and inp.fw[0] == 0.0
    assert not inp.onehot[inp.labels == -1].any() and not inp.onehot[inp.labels == c.cols].any()
    assert not inp.soft[1].any() and list(inp.soft[2, :2]) == [0.25, 0.75]
    for (target, sm), r in res.items():
        print("xent %-14s %-6s softmax %d: diff %.1e/%.1e  posteriors %.1e/%.1e  sums %s" % ((name, target, sm) + r["d_diff"] + r["d_post"] + (r["sums"],)))
        # (an fp32 softmax adds up to 8192 terms one after the other: 1e-5 is sqrt(8192) half-ulps, twice over)
        assert r["d_diff"][0] < 1e-5 and r["d_diff"][1] < 1e-5 and r["d_post"][0] < 1e-5 and r["d_post"][1] < 1e-5
        assert r["orc_sums"][0] == r["sums"][0] and r["orc_sums"][1] == r["sums"][1], (target, sm, r["orc_sums"], r["sums"])   # frames, correct: exact
        assert np.allclose(r["orc_sums"], r["sums"], rtol=1e-5, atol=1e-6)
        if c.rows >= 8:                               # some rows are classified correctly, some are not
            assert 0 < r["sums"][1] < r["sums"][0]
        off = (inp.onehot if target == "onehot" else inp.soft).sum(1) == 0
        assert off.sum() >= 2 and not r["diff"][off].any() and not r["diff"][0].any()      # switched-off rows, and the row of weight 0
