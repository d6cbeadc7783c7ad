"""The CuMatrix substrate kernels -- csrc/ew_kernels.hip (all but the *_p planes kernels and copy_mat_trans, which have their files),
csrc/conv_pool.hip, the non-softmax half of csrc/reduce_kernels.hip, csrc/optim_kernels.hip -- every entry point and every access path the host
code can pick, through the C ABI, element by element against the float64 models of tests/substrate_ref.py (pinned to the reference's own
library and held to the bars by tests/test_substrate_ref_cpu.py).

Every operand is a view into a wider buffer: inputs are padded with NaN, outputs and in-place operands with a sentinel that must still be
there afterwards, a destination the kernel promises not to read (beta == 0, the out-of-place maps) is NaN throughout.  launch_map operations
and the row gathers run on the access-path grid of substrate_ref.GRID (scalar, 16-byte, a pitch that is no multiple of 4, a base 4 bytes off,
a misaligned source alone, both paths into a grid-stride iteration, rows == 0 and cols == 0); which path a case takes is worked out here from
the host's own predicate on the pointers and strides actually passed, and test_every_path_was_reached holds the table to what it names.

The bars (none taken from the GPU) are the three classes of substrate_ref: bit-exact; k x 2^-24 x S with k the roundings counted in the
kernel's expression; library functions within max(3 x numpy-float32's own distance, 2 ulp) of float64 and 1e-4 on top.

MEASURED on an MI355X (599 tests: the 574 table cases, 5 max_norm_rows shapes, 18 solver runs, the refusals and the closing test; none
skipped, every named path reached), as test_every_path_was_reached prints it.  Library functions, worst distance to float64 in float32 ulps and
the case (bar: max(3 x numpy-float32's own worst, 2)):
    logf        2.10  apply_log-37x53-ld53            (bar 8.1; numpy's own 2.7)
    expf        0.78  apply_exp-37x53-ld53            (bar 6.0)
    powf        1.19  apply_pow-33x64-ld67            (bar 2.9)
    sqrtf       0.50  apply_pow_half-37x53-ld53       (bar 2.0: correctly rounded)
    sigmoid_ref 2.38  sigmoid-1030x2048-ld2048        (bar 10.5)
    tanh_ref    1.50  tanh-1030x2048-ld2048           (bar 7.2).  A deviation from "ulps of the float64 result": tanh_ref is counted in ulps of
                      max(|result|, 1), because it forms 1 - q with q in [1, 2] and its error is absolute (substrate_ref.ULP_FLOOR).  That is
                      the tighter reading: near zero, ulps of the result would let anything up to the 1e-4 ceiling pass.
    group pnorm 4.00  group_pnorm-g1-p3               (bar 9.3; powf twice, the second with the float32 1 / 3)
    pnorm deriv 2.57  group_pnorm-g10-p3              (bar 6.3)
Derived bounds, largest fraction used: 0.993 over the table (add_mat_mat_elements_beta0-1030x2048, k = 2: two roundings nearly aligned; the same
0.993 comes out of the numpy-float32 evaluation of that case), 0.68 over the solver steps (adam, n = 524,325).  max_norm_rows: the largest row
norm afterwards is max_norm (1 + 2.15 x 2^-24) (8200 x 64), inside the 4.  Every bit-exact class matched, padding and inputs untouched, all 49
refusals refused and the seven unmodified calls behind them accepted.
The file takes 5.5 s, 2.4 s of it in the table cases; the slowest test is add_mat-1030x2048-ld2048 at 0.17 s; the largest operand, the
33 MB of add_col_sum_mat_vec at 8200 x 1000, takes 0.13 s.
Nothing was found wrong in a kernel: all cases pass on the kernels as they stand, and no .hip file changed with this file.
A library with the ten small in-bounds changes of devtools/substrate_mutations.py -- map_vec4's second lane passing column c for c + 1,
add_rows' fourth lane adding v.z, the last of several patches dropped from the conv in-diff, the max-pool reset at -1e30, the last column of a
row wider than 64 dropped from add_col_sum_mat_vec, Adam without its second correction, d2f truncating, the p-norm without its rescale branch,
the scatter ignoring column 0, splice backward clamping one row early -- fails 55 of the 599 tests in one run, and each change fails at least
one of them (mul_cols_vec 3, add_vec_to_rows 5, add_mat_diag_vec 3, on the 16-byte cases only; add_rows 3; conv_in_diff 4; max_pool 5;
col_sum 16; adam 2; d2f 4; group_pnorm p = 3 4; scatter_add 1; splice_backward 5).
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import substrate_ref as R
from substrate_ref import f32, f64

pytestmark = pytest.mark.gpu
TABLE = R.table()
REFUSALS = ("bad arguments", "must be > 0", "unknown solver")
_t0 = time.time()
launch_failed = []          # [(what, error)]: once a launch ended in an error, nothing further is started on the GPU
reached = {}                # (op, path) -> cases
worst = {}                  # class -> (fraction of the bar used / ulp distance, case)
seconds = {}


def on_gpu(aslp, what, fn):
    """fn() behind the guard, then the library's error check, a synchronize and the check again: an error other than a refused argument stops
    every later GPU call of this file"""
    if launch_failed:
        pytest.fail("not started: %s ended in an error, and nothing more runs on the GPU behind it\n%s" % launch_failed[0])
    try:
        out = fn()
        aslp.ops.check_error()
        torch.cuda.synchronize()
        aslp.ops.check_error()
        return out
    except RuntimeError as e:
        if not any(r in str(e) for r in REFUSALS):
            launch_failed.append((what, repr(e)))
        raise
    except AssertionError:
        raise
    except Exception as e:
        launch_failed.append((what, repr(e)))
        raise


class OnDevice:
    """the operands of a case on the device: name -> buffer; p(name) the pointer to the view, d(name) its MatrixDim"""

    def __init__(self, aslp, dev, ops):
        if launch_failed:           # no copy to the device either, once a launch has failed
            pytest.fail("not started: %s ended in an error, and nothing more runs on the GPU behind it\n%s" % launch_failed[0])
        self.ops, self.md = ops, aslp._lib.MatrixDim
        self.t = {n: torch.from_numpy(o.image.copy()).to(dev) for n, o in ops.items()}

    def addr(self, n):
        return self.t[n].data_ptr() + self.ops[n].start * self.ops[n].dtype.itemsize

    def p(self, n):
        return C.c_void_p(self.addr(n))

    def d(self, n):
        o = self.ops[n]
        return self.md(o.rows, o.cols, o.ld)

    def ld(self, n):
        return self.ops[n].ld

    def back(self, n):
        return self.t[n].cpu().numpy()

    def vec(self, cols, names):
        """the host's 16-byte predicate on the pointers and strides as passed"""
        return R.vec_path(cols, [(self.addr(n), self.ops[n].ld) for n in names])


def note(cls, used, cid):
    if not used <= worst.get(cls, (0.0, ""))[0]:
        worst[cls] = (used, cid)


def check_outputs(c, g, expect=None, fails=None):
    fails = [] if fails is None else fails
    for k, exp in (expect or c.expect).items():
        f, (cls, used) = R.judge(c.ops[k] if k in c.ops else g.ops[k], g.back(k), exp, "%s %s" % (c.id, k))
        note(cls, used, c.id)
        fails += f
    for k, o in g.ops.items():          # inputs: nothing may have been written
        if o.is_input and k not in (expect or c.expect) and not np.array_equal(R._bits(g.back(k)), R._bits(o.image)):
            fails.append("%s: the input %s was written" % (c.id, k))
    return fails


def _d3(aslp, x=1, y=1, z=1):
    return aslp._lib.Dim3(x, y, z)


def call_map(aslp, c, g):
    lib, n, p, D = aslp.lib, c.op, c.par, _d3(aslp)
    d, P = g.d("dst"), g.p
    if n in ("set_const", "add", "scale", "apply_floor", "apply_ceiling"): getattr(lib, "cudaF_" + n)(D, D, P("dst"), p["v"], d)
    elif n.startswith("apply_pow"): lib.cudaF_apply_pow(D, D, P("dst"), p["v"], d)
    elif n in ("apply_log", "apply_exp", "apply_heaviside", "invert_elements"): getattr(lib, "cudaF_" + n)(D, D, P("dst"), d)
    elif n == "apply_clamp": lib.aslp_apply_clamp(P("dst"), d, p["lo"], p["hi"])
    elif n == "mul_elements": lib.cudaF_mul_elements(D, D, P("dst"), P("a"), d, g.ld("a"))
    elif n in ("mul_cols_vec", "mul_rows_vec"): getattr(lib, "cudaF_" + n)(D, D, P("dst"), P("v"), d)
    elif n == "add_mat": lib.cudaF_add_mat(D, D, p["alpha"], P("a"), P("dst"), d, g.ld("a"), 0)
    elif n == "add_vec_to_cols": lib.cudaF_add_vec_to_cols(D, D, p["alpha"], P("v"), p["beta"], P("dst"), d)
    elif n.startswith("add_vec_to_rows"): lib.cudaF_add_vec_to_rows(D, D, p["alpha"], P("v"), p["beta"], P("dst"), d)
    elif n == "add_mat_diag_vec": lib.cudaF_add_mat_diag_vec(D, D, p["alpha"], P("dst"), d, P("a"), g.ld("a"), 1, P("v"), p["beta"])
    elif n.startswith("add_mat_mat_elements"): lib.cudaF_add_mat_mat_elements(D, D, P("dst"), P("a"), P("b"), d, g.ld("a"), g.ld("b"), p["alpha"], p["beta"])
    elif n in ("sigmoid", "tanh"): getattr(lib, "cudaF_" + n)(D, D, P("dst"), P("a"), d, g.ld("a"))
    elif n in ("diff_sigmoid", "diff_tanh"): getattr(lib, "cudaF_" + n)(D, D, P("dst"), P("a"), P("b"), d, g.ld("a"), g.ld("b"))
    elif n == "diff_relu": lib.aslp_diff_relu(P("dst"), P("a"), P("b"), d, g.ld("a"), g.ld("b"))
    elif n == "copy_mat": lib.aslp_copy_mat(P("dst"), d, P("a"), g.ld("a"))
    else: raise KeyError(n)
    o = c.ops["dst"]
    vec = g.vec(o.cols, [k for k in c.ops if k != "v"])
    return R.path_name(vec, o.rows * (o.cols // 4 if vec else o.cols))


def call_other(aslp, c, g):
    """the launch of a case that is no launch_map operation -> the path the host's predicate picks for these pointers (None: the case's own)"""
    lib, n, p, D, P = aslp.lib, c.op, c.par, _d3(aslp), g.p
    if n in ("copy_rows", "add_rows", "randomize"):
        if n == "copy_rows": lib.cudaF_copy_rows(D, D, P("dst"), P("src"), P("idx"), g.d("dst"), g.ld("src"))
        elif n == "add_rows": lib.cudaF_add_rows(D, D, p["alpha"], P("dst"), P("src"), P("idx"), g.d("dst"), g.ld("src"))
        else: lib.cudaF_randomize(D, D, P("dst"), P("src"), P("idx"), g.d("dst"), g.d("src"))
        o = c.ops["dst"]
        vec = g.vec(o.cols, ["dst", "src"])
        return R.path_name(vec, o.rows * (o.cols // 4 if vec else o.cols))
    if n == "add_mat_trans": lib.cudaF_add_mat(D, D, p["alpha"], P("src"), P("dst"), g.d("dst"), g.ld("src"), 1)
    elif n == "add_mat_diag_vec_strided": lib.cudaF_add_mat_diag_vec(D, D, p["alpha"], P("dst"), g.d("dst"), P("m2"), 1, g.ld("m2"), P("v"), p["beta"])
    elif n == "regularize_l1": lib.cudaF_regularize_l1(D, D, P("w"), P("g"), p["l1"], p["lr"], g.d("w"), g.ld("g"))
    elif n == "copy_cols": lib.cudaF_copy_cols(D, D, P("dst"), P("src"), P("idx"), g.d("dst"), g.ld("src"))
    elif n == "add_cols": lib.cudaF_add_cols(D, D, P("dst"), P("src"), P("idx"), g.d("dst"), g.ld("src"))
    elif n == "copy": lib.cudaF_copy(D, D, P("dst"), P("src"), P("idx"), g.d("dst"), g.d("src"))
    elif n == "splice":
        lib.cudaF_splice(D, D, P("y"), P("x"), P("off"), g.d("y"), g.d("x"))
        return R.path_name(g.vec(c.ops["x"].cols, ["y", "x"]), 0)
    elif n == "splice_backward":
        lib.aslp_splice_backward(P("in_diff"), g.d("in_diff"), P("od"), g.ld("od"), P("off"), p["n_off"])
        return R.path_name(g.vec(c.ops["in_diff"].cols, ["in_diff", "od"]), 0)
    elif n == "set_const_i32": lib.cudaI32_set_const(D, D, P("dst"), p["v"], g.d("dst"))
    elif n == "scatter_add": lib.aslp_scatter_add(P("dst"), g.d("dst"), P("rows"), P("cols"), P("vals"), p["n"])
    elif n == "f2d": lib.aslp_f2d(P("dst"), P("src"), p["n"])
    elif n == "d2f": lib.aslp_d2f(P("dst"), P("src"), p["n"])
    elif n == "add_vec_vec": lib.cudaF_add_vec_vec(1, 1, p["alpha"], P("v"), P("x"), P("y"), p["beta"], p["n"])
    elif n == "vec_axpy": lib.aslp_vec_axpy(p["alpha"], P("x"), P("y"), p["n"])
    elif n == "vec_axpy2": lib.aslp_vec_axpy2(p["alpha"], P("x1"), P("y1"), P("x2"), P("y2"), p["n"])
    elif n == "vec_diff": lib.aslp_vec_diff(P("out"), P("a"), P("b"), p["n"])
    elif n == "dropout":
        lib.aslp_dropout_forward(P("out"), g.ld("out"), P("in"), g.d("in"), P("mask"), g.ld("mask"), p["retention"], p["seed"])
        lib.aslp_dropout_backward(P("in_diff"), g.ld("in_diff"), P("od"), g.d("od"), P("mask"), g.ld("mask"), p["retention"])
    elif n == "conv_gather": lib.aslp_conv_gather_patches(P("patches"), g.ld("patches"), P("in"), g.d("in"), p["P"], p["ns"], p["pd"], p["step"], p["stride"])
    elif n == "conv_in_diff": lib.aslp_conv_in_diff(P("in_diff"), g.d("in_diff"), P("patch_diff"), g.ld("patch_diff"), p["P"], p["ns"], p["pd"], p["step"], p["stride"])
    elif n == "max_pool":
        lib.aslp_max_pool_forward(P("out"), g.ld("out"), P("in"), g.d("in"), p["size"], p["step"], p["stride"])
        lib.aslp_max_pool_backward(P("in_diff"), g.ld("in_diff"), P("in"), g.d("in"), P("out"), g.ld("out"), P("od"), g.ld("od"), p["size"], p["step"], p["stride"])
    elif n == "length_norm": lib.aslp_length_norm_forward(P("out"), g.ld("out"), P("in"), g.d("in"), P("scales"))
    elif n == "group_pnorm": lib.cudaF_group_pnorm(D, D, P("y"), P("x"), g.d("y"), g.ld("x"), p["group"], p["power"])
    elif n == "group_max": lib.cudaF_group_max(D, D, P("y"), P("x"), g.d("y"), g.ld("x"), p["group"])
    elif n == "max": lib.cudaF_max(D, D, P("mat"), P("A"), g.d("mat"), g.ld("A"))
    elif n == "equal_element_mask": lib.cudaF_equal_element_mask(D, D, P("m1"), P("m2"), P("mask"), g.d("m1"), g.ld("m2"), g.ld("mask"))
    elif n == "mul_rows_group_mat": lib.cudaF_mul_rows_group_mat(D, D, P("y"), P("x"), g.d("y"), g.ld("x"), p["group"])
    elif n == "add_col_sum_mat_vec": lib.aslp_add_col_sum_mat_vec(p["alpha"], P("M"), g.d("M"), p["beta"], P("v"))
    elif n == "add_row_sum_mat_vec":
        lib.aslp_add_row_sum_mat_vec(p["alpha"], P("M"), g.d("M"), p["beta"], P("v"))
        return R.path_name(g.vec(c.ops["M"].cols, ["M"]), 0)
    elif n == "add_row_sum_mat_vec_sgd":
        lib.aslp_add_row_sum_mat_vec_sgd(p["alpha"], P("M"), g.d("M"), p["beta"], P("v"), P("w"), p["w_alpha"])
        return R.path_name(g.vec(c.ops["M"].cols, ["M"]), 0)
    elif n == "matrix_sum": lib.aslp_matrix_sum(P("M"), g.d("M"), P("out"))
    elif n == "vec_sum": lib.cudaF_vec_sum(1, 1, P("v"), P("value"), p["dim"], p["inc"])
    elif n == "add_diag_mat_mat":
        m_rs, m_cs = (1, g.ld("M")) if p["trans"] == 1 else (g.ld("M"), 1)
        n_rs, n_cs = (1, g.ld("N")) if p["trans"] == 2 else (g.ld("N"), 1)
        lib.cudaF_add_diag_mat_mat(1, 1, p["alpha"], P("v"), c.ops["v"].cols, P("M"), p["n"], m_rs, m_cs, P("N"), n_rs, n_cs, 1, p["beta"])
    elif n == "add_row_sum_mat":
        lib.cudaF_add_row_sum_mat(D, D, P("dst"), P("src"), g.d("dst"), g.ld("src"), p["P"], p["alpha"], p["beta"])
        return R.path_name(g.vec(c.ops["dst"].cols, ["dst", "src"]), 0)
    elif n == "add_conv_mat_mat_elements":
        lib.cudaF_add_conv_mat_mat_elements(D, _d3(aslp, 2, p["C"], 1), P("dst"), P("A"), P("B"), g.d("dst"), g.ld("A"), g.ld("B"), p["alpha"], p["beta"])
    else:
        raise KeyError(n)
    return None


@pytest.mark.parametrize("i", range(len(TABLE)), ids=[t[0] for t in TABLE])
def test_case(aslp, dev, i):
    t = time.time()
    c = TABLE[i][1]()
    g = OnDevice(aslp, dev, c.ops)
    path = on_gpu(aslp, c.id, lambda: (call_map if c.op in R.MAP_OPS else call_other)(aslp, c, g))
    path = c.path if path is None else path
    assert path == c.path, "%s: the host's predicate picks %s for these pointers, the table names %s" % (c.id, path, c.path)
    fails = check_outputs(c, g)
    empty = any(o.rows == 0 or o.cols == 0 for k, o in c.ops.items() if k in c.expect)
    reached.setdefault((c.op, "empty" if empty else path), []).append(c.name)
    if c.op == "length_norm":       # out == fl(x * scale) bit for bit from the scales as returned
        sc = c.ops["scales"].view(g.back("scales"))[0]
        f, _ = R.judge(c.ops["out"], g.back("out"), R.bits(R.length_norm_out(c.ops["in"].data(), sc)), c.id + " out")
        fails += f
        if c.ops["in"].rows >= 3:   # the zero row, through the reference's sequence of operations evaluated in numpy
            with np.errstate(all="ignore"):
                zs = f32(1) / np.sqrt(f32((c.ops["in"].data()[1] ** 2).sum()))
                zo = c.ops["in"].data()[1] * zs
            out = c.ops["out"].view(g.back("out"))
            assert np.array_equal(R._bits(sc[1:2]), R._bits(np.array([zs], f32))) and np.array_equal(R._bits(out[1]), R._bits(zo.astype(f32)))
    if c.op == "dropout":
        m = c.ops["mask"].view(g.back("mask"))
        assert set(np.unique(m)) <= {0.0, 1.0}
        if m.size >= 1000:          # the kept share within 6 binomial standard deviations
            q = c.par["retention"]
            assert abs(m.mean() - q) <= 6 * np.sqrt(q * (1 - q) / m.size), (m.mean(), q)
    if c.deriv:
        fails += group_backward(aslp, dev, c)
    seconds[c.id] = time.time() - t
    assert not fails, "\n".join(fails[:10])


def group_backward(aslp, dev, c):
    """calc_*_deriv against its model; then aslp_group_*_backward with a pitched out-diff against the two-launch sequence (calc_*_deriv,
    mul_rows_group_mat), bit for bit"""
    lib, D, dv, grp = aslp.lib, _d3(aslp), c.deriv, c.par["group"]
    ops = {"x": dv["x"], "y": dv["y"], "d": dv["d"], "od": dv["od"], "fused": R.Operand(dv["d"].data(), dv["d"].ld + 3, 1, R.SENTINEL)}
    g = OnDevice(aslp, dev, ops)
    mx = c.op == "group_max"

    def run():
        if mx:
            lib.cudaF_calc_group_max_deriv(D, D, g.p("d"), g.p("x"), g.p("y"), g.d("d"), g.ld("y"), grp)
        else:
            lib.cudaF_calc_pnorm_deriv(D, D, g.p("d"), g.p("x"), g.p("y"), g.d("d"), g.ld("y"), grp, c.par["power"])
    on_gpu(aslp, c.id + " deriv", run)
    fails = check_outputs(c, g, {"d": dv["expect"]})
    if dv["d"].ld != dv["x"].ld:
        return fails + ["calc_*_deriv reads x1 with the pitch of y: the case must give them one pitch"]

    def run2():
        lib.cudaF_mul_rows_group_mat(D, D, g.p("d"), g.p("od"), g.d("d"), g.ld("od"), grp)
        if mx:
            lib.aslp_group_max_backward(g.p("fused"), g.ld("fused"), g.p("x"), g.d("x"), g.p("y"), g.ld("y"), g.p("od"), g.ld("od"), grp)
        else:
            lib.aslp_group_pnorm_backward(g.p("fused"), g.ld("fused"), g.p("x"), g.d("x"), g.p("y"), g.ld("y"), g.p("od"), g.ld("od"), grp, c.par["power"])
    on_gpu(aslp, c.id + " backward", run2)
    two = ops["d"].view(g.back("d"))
    f, _ = R.judge(ops["fused"], g.back("fused"), R.bits(two), c.id + " fused backward against the two launches")
    return fails + f


@pytest.mark.parametrize("rows,cols", R.MAX_NORM_SHAPES)
def test_max_norm_rows(aslp, dev, rows, cols):
    x = R.max_norm_input(rows, cols)
    op = R.Operand(x, cols + 3, 1, R.SENTINEL)
    g = OnDevice(aslp, dev, {"W": op})
    on_gpu(aslp, "max_norm_rows", lambda: aslp.lib.aslp_max_norm_rows(g.p("W"), g.d("W"), R.MAX_NORM))
    img = g.back("W")
    after = op.view(img).copy()
    fails = R.max_norm_judge(op, img, x)
    reached.setdefault(("max_norm_rows", "gs" if rows > 2048 * 4 else "one"), []).append("%dx%d" % (rows, cols))
    nb = np.sqrt((after.astype(f64) ** 2).sum(axis=1)).max()
    note("max-norm: (largest row norm / max_norm - 1) / 2^-24", float((nb / R.MAX_NORM - 1) / R.U), "%dx%d" % (rows, cols))
    assert not fails, fails


@pytest.mark.parametrize("n", R.SOD_N)
@pytest.mark.parametrize("solver", R.SOLVERS)
def test_sod_solve(aslp, dev, solver, n):
    """two consecutive steps carrying state; the second step is checked from the state the first one left on the device"""
    grads, p0, s1, s2 = R.sod_inputs(solver, n)
    ops = {"param": R.Operand(p0, None, 1, R.SENTINEL), "prev": R.Operand(np.full(n, R.NAN, f32), None, 0, R.SENTINEL), "s1": R.Operand(s1, None, 1, R.SENTINEL),
           "s2": R.Operand(s2, None, 0, R.SENTINEL), "g0": R.Operand(grads[0], None, 0, R.NAN), "g1": R.Operand(grads[1], None, 1, R.NAN)}
    g = OnDevice(aslp, dev, ops)
    a = aslp._lib.SodSolver(R.SOLVERS.index(solver), *[R.SOD_PAR[k] for k in ("lr", "momentum", "gamma", "beta1", "beta2", "corr1", "corr2")])
    state = dict(param=p0, s1=s1, s2=s2)
    fails = []
    for step in (0, 1):
        on_gpu(aslp, "sod %s" % solver, lambda: aslp.lib.aslp_sod_solve(C.byref(a), g.p("g%d" % step), g.p("param"), g.p("prev"), g.p("s1"), g.p("s2"), n))
        ref = R.sod_step(solver, grads[step], state["param"], state["s1"], state["s2"])
        for k in ("param", "s1", "s2"):
            exp = R.bound(*ref[k]) if k in ref else R.bits(state[k])           # a state vector the solver does not use stays as it was
            f, (cls, used) = R.judge(ops[k], g.back(k), exp, "%s n=%d step %d %s" % (solver, n, step, k))
            note("solver " + cls, used, "%s-%d" % (solver, n))
            fails += f
        state = {k: ops[k].view(g.back(k))[0].copy() for k in ("param", "s1", "s2")}
        f, _ = R.judge(ops["prev"], g.back("prev"), R.bits(state["param"]), "%s prev" % solver)
        fails += f
    if solver != "sgd":
        assert (state["s1"][::5] == 0).all() or solver in ("momentum", "adam")      # zero gradients: the accumulator stayed 0, the floor was what the root saw
    reached.setdefault(("sod_solve", solver), []).append(n)
    assert not fails, "\n".join(fails[:10])


def refusal_calls(aslp, g):
    """(entry point, clause, call) -- one per clause of each argument check of csrc/conv_pool.hip that returns before any launch.  Only checked
    arguments are made wrong: no pointer a kernel would use is passed wrong, and no null where the entry point does not test for it"""
    lib, md, P, NULL = aslp.lib, aslp._lib.MatrixDim, g.p, C.c_void_p(0)
    o, i = P("out"), P("in")
    calls = []

    def vary(name, fn, base, clauses):
        calls.append((name, None, lambda: fn(*base)))      # the call as it stands is valid, and in bounds of the four 24 x 36 operands
        for what, idx, val in clauses:
            a = list(base); a[idx] = val
            calls.append((name, what, lambda a=a: fn(*a)))
    d = md(3, 33, 40)      # 3 splices of stride 10 (+3), patch_dim 4, step 1, 7 patches
    vary("aslp_conv_gather_patches", lib.aslp_conv_gather_patches, [o, 40, i, d, 7, 3, 4, 1, 10],
         [("patches null", 0, NULL), ("in null", 2, NULL), ("num_splice", 5, 0), ("patch_dim", 6, 0), ("patch_step", 7, 0), ("patch_stride", 8, 0), ("splices wider than the input", 5, 4),
          ("patches beyond the stride", 4, 8), ("ldp", 1, 11)])
    d = md(3, 30, 40)
    vary("aslp_conv_in_diff", lib.aslp_conv_in_diff, [o, d, i, 40, 7, 3, 4, 1, 10],
         [("in_diff null", 0, NULL), ("patch_diff null", 2, NULL), ("num_splice", 5, 0), ("patch_dim", 6, 0), ("patch_step", 7, 0), ("patch_stride", 8, 0), ("width", 1, md(3, 31, 40)),
          ("patches beyond the stride", 4, 8), ("ldp", 3, 11)])
    d = md(3, 30, 40)      # 10 patches of stride 3
    vary("aslp_max_pool_forward", lib.aslp_max_pool_forward, [o, 40, i, d, 3, 1, 3],
         [("out null", 0, NULL), ("in null", 2, NULL), ("pool_size", 4, 0), ("pool_step", 5, 0), ("pool_stride", 6, 0), ("stride does not divide", 6, 4), ("pool larger than the input", 4, 11)])
    vary("aslp_max_pool_backward", lib.aslp_max_pool_backward, [o, 40, i, d, P("a"), 40, P("b"), 40, 3, 1, 3],
         [("in_diff null", 0, NULL), ("in null", 2, NULL), ("out null", 4, NULL), ("out_diff null", 6, NULL), ("pool_size", 8, 0), ("pool_step", 9, 0), ("pool_stride", 10, 0),
          ("stride does not divide", 10, 4), ("pool larger than the input", 8, 11)])
    vary("aslp_length_norm_forward", lib.aslp_length_norm_forward, [o, 40, i, d, P("a")], [("out null", 0, NULL), ("in null", 2, NULL), ("row_scales null", 4, NULL)])
    vary("aslp_group_pnorm_backward", lib.aslp_group_pnorm_backward, [o, 40, i, d, P("a"), 40, P("b"), 40, 5, 2.0],
         [("in_diff null", 0, NULL), ("in null", 2, NULL), ("out null", 4, NULL), ("group_size", 8, 0), ("group does not divide", 8, 4)])
    vary("aslp_group_max_backward", lib.aslp_group_max_backward, [o, 40, i, d, P("a"), 40, P("b"), 40, 5],
         [("in_diff null", 0, NULL), ("in null", 2, NULL), ("out null", 4, NULL), ("group_size", 8, 0), ("group does not divide", 8, 4)])
    return calls


def test_refusals(aslp, dev):
    """every clause sets the library error with the entry point's name and leaves the sentinel everywhere; afterwards the unmodified call of
    each entry point is accepted, so each refusal was its own clause's"""
    ops = {k: R.Operand(np.full((24, 36), R.SENTINEL, f32), 40, 0, R.SENTINEL) for k in ("out", "in", "a", "b")}
    g = OnDevice(aslp, dev, ops)
    calls = refusal_calls(aslp, g)
    lib, D = aslp.lib, _d3(aslp)
    calls.append(("add_conv_mat_mat_elements", "Bl.y == 0", lambda: lib.cudaF_add_conv_mat_mat_elements(D, _d3(aslp, 2, 0, 1), g.p("out"), g.p("a"), g.p("b"), g.d("out"), 40, 40, 1.0, 0.0)))
    a = aslp._lib.SodSolver(6, 0.01, 0.9, 0.95, 0.9, 0.999, 1.0, 1.0)
    calls.append(("aslp_sod_solve", "unknown solver", lambda: lib.aslp_sod_solve(C.byref(a), g.p("a"), g.p("out"), g.p("in"), g.p("b"), g.p("b"), 8)))
    base = [c for c in calls if c[1] is None]
    calls = [c for c in calls if c[1] is not None]
    assert len(calls) == 9 + 9 + 7 + 9 + 3 + 5 + 5 + 2 and len(base) == 7
    for name, what, fn in calls:
        with pytest.raises(RuntimeError) as e:
            on_gpu(aslp, "%s: %s" % (name, what), fn)
        assert name in str(e.value), (name, what, str(e.value))
        assert not launch_failed, launch_failed
    for k, o in ops.items():
        assert np.array_equal(R._bits(g.back(k)), R._bits(o.image)), k
    for name, _, fn in base:
        on_gpu(aslp, name + " as it stands", fn)
    reached[("refusals", "refused")] = [len(calls)]


def test_every_path_was_reached(dev):
    got = {}
    for (op, path), cases in reached.items():
        got.setdefault(op, set()).add(path)
    print("\nworst distances (fraction of the derived bound used; float32 ulps for a library function):")
    for cls in sorted(worst):
        print("    %-28s %10.3f   %s" % ((cls,) + worst[cls]))
    slow = max(seconds.items(), key=lambda kv: kv[1]) if seconds else ("-", 0.0)
    print("    %.1f s since the file was imported, %.1f s in the table cases; slowest %s at %.2f s" % (time.time() - _t0, sum(seconds.values()), slow[0], slow[1]))
    assert not launch_failed, launch_failed
    for op in list(R.MAP_OPS) + ["copy_rows", "add_rows", "randomize"]:
        want = {"scalar", "vec4", "empty"} | (set() if op in R.UNARY_INPLACE and op not in R.BIG_UNARY else {"scalar-gs", "vec4-gs"})
        assert got.get(op) == want, (op, got.get(op))
    for op in ("splice", "splice_backward", "add_row_sum_mat", "add_row_sum_mat_vec_sgd", "add_row_sum_mat_vec"):
        assert got.get(op) == {"scalar", "vec4"}, (op, got.get(op))
    for op in ("conv_gather", "conv_in_diff", "length_norm", "add_col_sum_mat_vec", "max_norm_rows"):
        assert got.get(op) == {"one", "gs"}, (op, got.get(op))
    assert len(reached[("add_col_sum_mat_vec", "gs")]) == 10      # 8200 rows at each of the five widths, beta 0 and 0.5
    assert got.get("matrix_sum") == {"one", "gs"} and got.get("vec_sum") == {"one"}
    assert got.get("max_pool") == {"covered", "uncovered"} and got.get("group_pnorm") == {"plain", "rescale"}
    assert got.get("sod_solve") == set(R.SOLVERS) and got.get("refusals") == {"refused"}
    assert len(reached) >= 100 and sum(len(v) for v in reached.values()) >= len(TABLE)
