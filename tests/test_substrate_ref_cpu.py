"""tests/substrate_ref.py, the checker of tests/test_substrate_kernels_gpu.py, checked without a GPU:
  * its models reproduce what the reference's own CuMatrix library gave (tests/golden/cumatrix_ops.bin, component_ops.bin) and the UnitTest*
    vectors of component_known_answers.json: index work bit-exact, the rest within the bound of its class;
  * a plain float32 evaluation of every table case -- separate roundings, and products folded into the adds -- lies inside the bar its GPU
    comparison uses (no bar is tighter than correct fp32 arithmetic), and LIB_NUMPY_WORST is what numpy's float32 functions measure there;
  * `judge` rejects a wrong kernel: two adjacent columns swapped, the last element zeroed, rows shifted down by one, one element moved by
    4 x its bound (one ulp where the class is bit-exact), one padding word overwritten -- on every table case where the mutation changes
    the output."""
import math

import numpy as np

import cumatrix_golden
import substrate_ref as R
from substrate_ref import f32, f64

TABLE = R.table()
_built = {}


def build(i):
    """the big cases are built once for the three tests that walk the table"""
    if i not in _built:
        _built[i] = TABLE[i][1]()
    return _built[i]


def outputs(c):
    """(operand, expectation, fp32 evaluations) of every output of a case"""
    items = [(k, c.ops[k], c.expect[k], [ev[k] for ev in c.evals]) for k in c.expect]
    if c.deriv:
        items.append(("deriv", c.deriv["d"], c.deriv["expect"], c.deriv["evals"]))
    return items


def filled(op, values):
    img = op.image.copy()
    op.view(img)[...] = np.asarray(values).astype(op.dtype).reshape(op.rows, op.cols)
    return img


def within(got, model64, k, S=None):
    """a stored reference output against a float64 model under the derived bound"""
    op = R.Operand(np.asarray(got))
    S = np.abs(model64) if S is None else S
    fails, _ = R.judge(op, op.image, R.bound(model64, k, S), "golden")
    return not fails


def fmodel(name, d, a=None, b=None, v=None, **par):
    """a launch_map functor in float64 and on the magnitudes -> (ref, S)"""
    f = R.MAP_OPS[name][3]
    return [f(A, *[A.x(t) if t is not None else None for t in (d, a, b, v)], par) for A in (R.ARITH[0], R.ARITH[3])]


def test_map_models_match_reference_library():
    g = cumatrix_golden.load()
    x, d, pos = g["x"], g["d"], g["pos"]
    F = R.ARITH[1]
    for name, args, par, want in (("apply_floor", (x,), dict(v=0.0), g["relu"]), ("apply_heaviside", (x,), {}, g["heaviside"]),
                                  ("apply_clamp", (x,), dict(lo=-1.5, hi=2.5), g["floor_ceil"]), ("mul_elements", (x, d), {}, g["mul_elements"]),
                                  ("apply_pow2", (x,), {}, g["pow2"]), ("mul_cols_vec", (g["bc_in"], None, None, g["bc_row"]), {}, g["mul_cols_vec"]),
                                  ("mul_rows_vec", (g["bc_in"], None, None, g["bc_col"].T), {}, g["mul_rows_vec"])):
        got = R.MAP_OPS[name][3](F, *[F.x(t) if t is not None else None for t in (list(args) + [None] * 3)[:4]], par)
        assert np.array_equal(R._bits(np.asarray(got, f32)), R._bits(want)), name
    for name, args, par, want in (("invert_elements", (pos,), {}, g["invert"]), ("diff_sigmoid", (None, d, g["sigmoid"]), {}, g["diff_sigmoid"]),
                                  ("diff_tanh", (None, d, g["tanh"]), {}, g["diff_tanh"]),
                                  ("add_mat_mat_elements", (g["mme_dst_in"], g["mme_A"], g["mme_B"]), dict(alpha=-1.25, beta=0.5), g["mme_dst_out"]),
                                  ("add_mat_diag_vec", (g["mdv_dst_in"], g["mdv_M"], None, g["mdv_vec"]), dict(alpha=0.75, beta=1.0), g["mdv_dst_out"]),
                                  ("add_mat_diag_vec", (g["mdv_dst_in_t"], g["mdv_Mt"].T, None, g["mdv_vec"]), dict(alpha=-0.5, beta=1.0), g["mdv_dst_out_t"]),
                                  ("add_vec_to_rows", (g["bc_in"], None, None, g["bc_row"]), dict(alpha=0.5, beta=1.0), g["add_vec_to_rows"]),
                                  ("add_vec_to_cols", (g["bc_in"], None, None, g["bc_col"].T), dict(alpha=-1.5, beta=1.0), g["add_vec_to_cols"])):
        args = (list(args) + [None] * 3)[:4]
        if args[0] is None: args[0] = np.zeros_like(want)
        ref, S = fmodel(name, *args, **par)
        assert within(want, ref, R.MAP_OPS[name][4], S), name
    for name, src, want, fn in (("apply_log", pos, g["log"], "log"), ("apply_exp", d, g["exp"], "exp"), ("sigmoid", x, g["sigmoid"], "sigmoid"), ("tanh", x, g["tanh"], "tanh")):
        args = (src, None, None) if name.startswith("apply") else (np.zeros_like(src), src, None)
        ref = fmodel(name, *args)[0]
        assert R.ulp_dist(want, ref, fn).max() <= R.lib_bar(fn) and np.abs(want - ref).max() <= 1e-4, name


def test_gather_and_composite_models_match_reference_library():
    g = cumatrix_golden.load()
    assert np.array_equal(R.splice_model(g["splice_in"], g["splice_off"]), g["splice_out"])
    idx = g["copy_cols"]
    assert np.array_equal(np.where(idx[None, :] < 0, f32(0), g["splice_in"][:, np.maximum(idx, 0)]), g["copy_out"])
    assert np.array_equal(g["splice_in"][g["rand_mask"]], g["randomize_out"])
    idx = g["cols_idx"]
    gathered = np.where(idx[None, :] < 0, f32(0), g["cols_in"][:, np.maximum(idx, 0)])
    assert np.array_equal(gathered, g["copy_cols_out"]) and np.array_equal((g["cols_dst_in"] + gathered).astype(f32), g["add_cols_out"])
    wo, go, margin = R.regularize_l1_model(g["l1_w_in"], g["l1_g_in"], 0.002, 0.01)
    sure = margin > 1e-6          # away from a rounding of the sign test
    assert np.array_equal(wo[sure], g["l1_w_out"][sure]) and np.array_equal(go[sure], g["l1_g_out"][sure]) and sure.mean() > 0.99
    A_, B_, C = g["conv_A"], g["conv_B"], g["conv_B"].shape[0]
    rows = np.arange(g["conv_dst_in"].shape[0])
    a, b = A_[rows // C + rows % C], B_[rows % C]
    ref, S = fmodel("add_mat_mat_elements", g["conv_dst_in"], a, b, alpha=0.7, beta=0.3)
    assert within(g["conv_dst_out"], ref, 4, S)
    ref, S = fmodel("add_mat_mat_elements_beta0", np.zeros_like(a), a, b, alpha=1.0, beta=0.0)
    assert within(g["conv_dst_beta0"], ref, 2, S)


def test_component_models_match_reference_library_and_unit_tests():
    g = cumatrix_golden.load_components()
    _, size, step, stride = [int(v) for v in g["pool_geom"]]
    out = R.maxpool_fwd_model(g["pool_in"], size, step, stride)
    assert np.array_equal(out, g["pool_out"])
    assert np.array_equal(R.maxpool_bwd_model(g["pool_in"], out, g["pool_od"], size, step, stride)[0], g["pool_id"])
    assert np.array_equal(np.where(g["op_max_b"] > g["op_max_a"], g["op_max_b"], g["op_max_a"]), g["op_max_out"])
    assert np.array_equal((g["op_max_a"] == g["op_max_b"]).astype(f32), g["op_eqmask"])
    for w in (0, 1):
        x = g["ln%d_in" % w]
        assert within(g["ln%d_scales" % w], R.length_norm_scales(R.ARITH[0], x), 3)
        assert np.array_equal(R.length_norm_out(x, g["ln%d_scales" % w]), g["ln%d_out" % w])
    x, od = g["grp_in"], g["grp_od"]
    group = x.shape[1] // od.shape[1]
    for i, p in enumerate((2.0, 1.0, 3.0)):
        y = R.group_pnorm_model(R.ARITH[0], x.astype(f64), group, p)
        assert R.ulp_dist(g["pnorm%d_out" % i], y).max() <= R.lib_bar("pnorm"), p
        dv = R.group_deriv_model(R.ARITH[0], x.astype(f64), g["pnorm%d_out" % i].astype(f64), group, p)
        assert R.ulp_dist(g["pnorm%d_deriv" % i], dv).max() <= R.lib_bar("pnorm_deriv"), p
        assert np.array_equal((g["pnorm%d_deriv" % i] * np.repeat(od, group, axis=1)).astype(f32), g["pnorm%d_id" % i])      # mul_rows_group_mat: one rounding
    y = x.reshape(x.shape[0], -1, group).max(axis=2)
    assert np.array_equal(y, g["gmax_out"]) and np.array_equal((x == np.repeat(y, group, axis=1)).astype(f32), g["gmax_deriv"])
    known = cumatrix_golden.load_known_answers()
    m = known["UnitTestMaxPoolingComponent"]["matrices"]
    assert np.array_equal(R.maxpool_fwd_model(m["mat_in"], 3, 3, 4), m["mat_out_ref"])
    m = known["UnitTestConvolutionalComponent3x3"]["matrices"]      # 9 filters outputs from 15 inputs: 3 x 3 filters, patch_dim 3, step 1, stride 5: 3 patches, 3 splices
    filt = np.array([[-1, -2, -7, 0, 0, 0, 1, 2, 7], [-1, 0, 1, -3, 0, 3, -2, 2, 0], [-4, 0, 0, -3, 0, 3, 4, 0, 0]], f64)
    patches = R.conv_gather_model(m["mat_in"].astype(f64), 3, 3, 1, 5, 3)
    assert np.array_equal((patches @ filt.T - 20).reshape(1, 9), m["mat_out_ref"])
    pdiff = m["mat_out_diff"].astype(f64).reshape(3, 3) @ filt
    assert np.array_equal(R.conv_indiff_model(pdiff, 3, 3, 1, 5, 3, f64), m["mat_in_diff_ref"])
    m = known["UnitTestConvolutionalComponentUnity"]["matrices"]["mat_in"]      # one filter [ 1 ] over five patches of one: the identity both ways
    patches = R.conv_gather_model(m, 1, 1, 1, 5, 5)
    assert np.array_equal(patches.reshape(1, 5), m) and np.array_equal(R.conv_indiff_model(patches, 1, 1, 1, 5, 5), m)
    m = known["UnitTestLengthNorm"]["matrices"]["mat_in"]
    out = R.length_norm_out(m, R.length_norm_scales(R.ARITH[1], m))
    assert np.allclose((out.astype(f64) ** 2).sum(axis=1), 1.0, atol=1e-6)


def test_conv_models_match_reference_library():
    """ConvolutionalComponent at the golden's 13 x 30 (3 splices of stride 10, patch_dim 4, step 2: 4 overlapping patches, 5 filters), two
    minibatches: conv_gather_model, then the product with the filters plus bias in float64, against conv_out*; the out-diff times the filters,
    then conv_indiff_model, against conv_id*.  The stored outputs went through a float32 product: k = its terms + 2 (the sum, the bias or the
    sum over patches), S the magnitudes"""
    g = cumatrix_golden.load_components()
    in_dim, F, pd, step, stride = [int(v) for v in g["conv_geom"][:5]]
    ns, P = in_dim // stride, 1 + (stride - pd) // step
    for i in (0, 1):
        filt, bias, x, od = (g["conv_%s%d" % (k, i)].astype(f64) for k in ("filters", "bias", "in", "od"))
        N = x.shape[0]
        patches = R.conv_gather_model(x, ns, pd, step, stride, P)
        assert np.array_equal(patches, R.conv_gather_model(g["conv_in%d" % i], ns, pd, step, stride, P))      # an index operation: the same in any type
        out = (patches @ filt.T + bias).reshape(N, P * F)                    # out[n][p F + f]
        S = (np.abs(patches) @ np.abs(filt).T + np.abs(bias)).reshape(N, P * F)
        assert within(g["conv_out%d" % i], out, ns * pd + 2, S), i
        pdiff, Sp = od.reshape(N * P, F) @ filt, np.abs(od).reshape(N * P, F) @ np.abs(filt)
        idf, Si = R.conv_indiff_model(pdiff, ns, pd, step, stride, P, f64), R.conv_indiff_model(Sp, ns, pd, step, stride, P, f64)
        assert within(g["conv_id%d" % i], idf, F + P + 2, Si), i
        # and the ordered float32 model on float32 patch diffs stays inside the same bound
        assert within(R.conv_indiff_model(pdiff.astype(f32), ns, pd, step, stride, P), idf, F + P + 2, Si), i
        dropped = R.conv_indiff_model(np.where(np.arange(N * P)[:, None] % P == P - 1, 0.0, pdiff), ns, pd, step, stride, P, f64)
        assert not within(dropped.astype(f32), idf, F + P + 2, Si)           # the last patch left out is far outside it


def round_up2(v):
    """v rounded up to two significant digits"""
    if v <= 0: return 0.0
    e = 10.0 ** (math.floor(math.log10(v)) - 1)
    return math.ceil(v / e - 1e-9) * e


def test_fp32_stays_within_every_bound_and_numpy_worst_is_as_stored():
    worst, used, bad = {}, {}, []
    for i, (cid, _) in enumerate(TABLE):
        c = build(i)
        for key, op, exp, evals in outputs(c):
            assert evals, cid
            for ev in evals:
                fails, (cls, u) = R.judge(op, filled(op, ev), exp, "%s %s" % (cid, key))
                if cls.startswith("ulp:"):
                    if u > worst.get(cls[4:], (0, ""))[0]: worst[cls[4:]] = (u, cid)
                    fails = [f for f in fails if "beyond" not in f]       # (the bar is made from this very distance, below)
                elif u > used.get(cls, (0, ""))[0]: used[cls] = (u, cid)
                bad += fails
    print("float32 evaluations: worst fraction of a derived bound %s; numpy-float32 ulp distances %s" % (used, worst))
    assert not bad, "\n".join(bad[:20])
    assert used["bound"][0] <= 1.0
    assert set(worst) <= set(R.LIB_NUMPY_WORST), worst
    # the stored figures are this machine class's; another build of numpy may pick other vector routines: within a factor of two, and no
    # stored figure above what a faithfully-rounded-class routine and a handful of roundings give
    for fn, (u, cid) in worst.items():
        assert u <= 2.0 * R.LIB_NUMPY_WORST[fn], (fn, u, cid, R.LIB_NUMPY_WORST[fn])
        assert R.LIB_NUMPY_WORST[fn] <= 1.5 * round_up2(u), (fn, u, cid, R.LIB_NUMPY_WORST[fn])       # nor may a stored figure drift above what is measured
    assert max(R.LIB_NUMPY_WORST.values()) <= 4.0
    print("rounded up to two digits:", {fn: round_up2(u) for fn, (u, _) in worst.items()})


def test_fp32_max_norm_and_solver_steps_stay_within_their_bars():
    seen = set()
    for rows, cols in R.MAX_NORM_SHAPES:
        x = R.max_norm_input(rows, cols)
        op, good = R.Operand(x, cols + 3, 1, R.SENTINEL), R.max_norm_f32(x)
        assert not R.max_norm_judge(op, filled(op, good), x), (rows, cols)
        bad = good.copy()
        bad[1] = x[1]                     # a row above the norm left as it was
        assert R.max_norm_judge(op, filled(op, bad), x)
        want = np.abs(good.astype(f64))
        for name, m in mutations(op, R.bound(want, 8, want), good):      # (the expectation only sizes the moved element: 4 x 8u of it)
            seen.add(name)
            assert R.max_norm_judge(op, m, x), (rows, cols, name)
    for solver in R.SOLVERS:
        for n in R.SOD_N:
            g, p, s1, s2 = R.sod_inputs(solver, n)
            for step in (0, 1):
                ref = R.sod_step(solver, g[step], p, s1, s2)
                new = sod_f32(solver, g[step], p, s1, s2)
                for k, (r, kk, S) in ref.items():
                    assert (np.abs(new[k] - r) <= kk * R.U * S).all(), (solver, n, step, k)
                    op, exp = R.Operand(new[k], None, 1, R.SENTINEL), R.bound(r, kk, S)      # as the GPU file judges it
                    assert not R.judge(op, filled(op, new[k]), exp)[0], (solver, n, step, k)
                    for name, m in mutations(op, exp, new[k]) if n <= 257 else ():
                        assert R.judge(op, m, exp)[0], (solver, n, step, k, name)
                p, s1, s2 = new["param"], new.get("s1", s1), new.get("s2", s2)
            assert (s1[::5] == 0).all() or solver in ("sgd",)
    assert seen == {"columns swapped", "last element zeroed", "rows shifted down", "one element moved", "padding overwritten"}


def sod_f32(solver, g, p, s1, s2, par=R.SOD_PAR):
    """the solvers in separate float32 roundings, in the kernel's order"""
    c = {k: f32(v) for k, v in par.items()}
    isf = lambda v: (f32(1) / np.sqrt(np.maximum(v, f32(1e-8))).astype(f32)).astype(f32)
    out = {}
    if solver == "sgd":
        out["param"] = (p + (-c["lr"] * g).astype(f32)).astype(f32)
    elif solver == "momentum":
        m = ((c["lr"] * g).astype(f32) + (c["momentum"] * s1).astype(f32)).astype(f32)
        out["s1"], out["param"] = m, (p - m).astype(f32)
    elif solver in ("adagrad", "rmsprop"):
        a, b = (f32(1), f32(1)) if solver == "adagrad" else (f32(0.1), f32(0.9))
        G = (((a * g).astype(f32) * g).astype(f32) + (b * s1).astype(f32)).astype(f32)
        out["s1"], out["param"] = G, (p + (-c["lr"] * (isf(G) * g).astype(f32)).astype(f32)).astype(f32)
    elif solver == "adadelta":
        om = f32(1) - c["gamma"]
        G = (((om * g).astype(f32) * g).astype(f32) + (c["gamma"] * s1).astype(f32)).astype(f32)
        step = ((isf(G) * np.sqrt(np.maximum(s2, f32(1e-8))).astype(f32)).astype(f32) * g).astype(f32)
        out["s1"], out["param"] = G, (p - step).astype(f32)
        out["s2"] = (((om * step).astype(f32) * step).astype(f32) + (c["gamma"] * s2).astype(f32)).astype(f32)
    else:
        o1, o2 = f32(1) - c["beta1"], f32(1) - c["beta2"]
        m = ((o1 * g).astype(f32) + (c["beta1"] * s1).astype(f32)).astype(f32)
        v = (((o2 * g).astype(f32) * g).astype(f32) + (c["beta2"] * s2).astype(f32)).astype(f32)
        out["s1"], out["s2"] = m, v
        out["param"] = (p + ((-c["lr"] * c["corr1"]) * (isf((v * c["corr2"]).astype(f32)) * m).astype(f32)).astype(f32)).astype(f32)
    return out


def mutations(op, exp, good):
    """(name, mutated buffer image) of every mutation that changes the buffer"""
    img = filled(op, good)
    v = lambda im: op.view(im)
    out = []
    if op.cols >= 2:
        m = img.copy()
        differ = R._bits(v(m)[:, :-1]) != R._bits(v(m)[:, 1:])
        r = next((r for r in list(range(op.rows // 2, op.rows)) + list(range(op.rows // 2)) if differ[r].any()), None)      # the first row from the middle with two unequal neighbours
        if r is not None:
            c = int(np.argmax(differ[r]))
            v(m)[r, [c, c + 1]] = v(m)[r, [c + 1, c]]
            out.append(("columns swapped", m))
    m = img.copy(); v(m)[-1, -1] = 0
    out.append(("last element zeroed", m))
    if op.rows >= 2:
        m = img.copy(); v(m)[1:] = v(img)[:-1]
        out.append(("rows shifted down", m))
    m = img.copy(); r, c = op.rows // 2, op.cols // 3
    if exp[0] == "bits":
        one = R._bits(v(m)[r, c:c + 1]); one += 1
    elif exp[0] == "bound":
        S = np.broadcast_to(exp[3], (op.rows, op.cols))[r, c]
        v(m)[r, c] += op.dtype.type(4.04 * exp[2] * exp[4] * max(S, 1e-30))
    else:
        v(m)[r, c] = v(m)[r, c] * op.dtype.type(1 + 4.04 * R.lib_bar(exp[2]) * 2.0 ** -23) + op.dtype.type(1e-37)
    out.append(("one element moved", m))
    m = img.copy()
    m[op.start + op.rows * op.ld + 1 if op.rows else 0] = op.dtype.type(1)      # a word behind the last row
    out.append(("padding overwritten", m))
    return [(n, m) for n, m in out if not np.array_equal(R._bits(m), R._bits(img))]


def test_judge_rejects_wrong_kernels():
    missed, seen = [], {}
    for i, (cid, _) in enumerate(TABLE):
        c = build(i)
        for key, op, exp, evals in outputs(c):
            if op.rows == 0 or op.cols == 0:
                continue
            good = evals[0] if exp[0] != "ulp" else exp[1].astype(f32)
            assert not R.judge(op, filled(op, good), exp)[0] or exp[0] == "ulp", cid
            for name, m in mutations(op, exp, good):
                seen[name] = seen.get(name, 0) + 1
                if exp[0] == "ulp" and name != "padding overwritten":
                    # a moved value has to differ from the right one by more than the bar to count as a wrong kernel's
                    g_, r_ = op.view(m), np.broadcast_to(exp[1], (op.rows, op.cols))
                    if R.ulp_dist(g_, r_, exp[2]).max() <= R.lib_bar(exp[2]):
                        continue
                if not R.judge(op, m, exp)[0]:
                    missed.append("%s %s: %s passes" % (cid, key, name))
    print("mutations applied:", seen)
    assert not missed, "\n".join(missed[:30])
    assert all(seen.get(n, 0) > 100 for n in ("columns swapped", "last element zeroed", "rows shifted down", "one element moved", "padding overwritten"))


def test_dropout_generator_and_paths():
    u = R.dropout_uniform(5, 256 * 512)
    assert u.min() >= 0 and u.max() < 1 and abs(u.mean() - 0.5) < 0.01
    assert not np.array_equal(R.dropout_uniform(11, 91), R.dropout_uniform(12, 91))
    paths = {}
    for i, (cid, _) in enumerate(TABLE):
        c = build(i)
        paths.setdefault(c.op, set()).add(c.path)
    for op in list(R.MAP_OPS) + ["copy_rows", "add_rows", "randomize"]:
        want = {"scalar", "vec4"} | (set() if op in R.UNARY_INPLACE and op not in R.BIG_UNARY else {"scalar-gs", "vec4-gs"})
        assert paths[op] == want, (op, paths[op])
    assert paths["splice"] == paths["splice_backward"] == paths["add_row_sum_mat"] == {"scalar", "vec4"}
    assert paths["conv_gather"] == paths["conv_in_diff"] == paths["length_norm"] == paths["add_col_sum_mat_vec"] == paths["matrix_sum"] == {"one", "gs"}
    assert sum(1 for i in range(len(TABLE)) if build(i).op == "add_col_sum_mat_vec" and build(i).path == "gs") == 10
    assert paths["max_pool"] == {"covered", "uncovered"} and paths["group_pnorm"] == {"plain", "rescale"}
