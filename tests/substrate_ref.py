"""numpy models of the CuMatrix substrate kernels (csrc/ew_kernels.hip, csrc/conv_pool.hip, the non-softmax half of csrc/reduce_kernels.hip,
csrc/optim_kernels.hip), the case tables of tests/test_substrate_kernels_gpu.py and one comparison (`judge`) per class of operation.

A model is written ONCE over an arithmetic object and evaluated four ways: F64 (the reference), F32 (every operation rounded to float32),
F32F (a product folded into the add that consumes it: float64 then one rounding, what contraction gives) and ABS (float64 on the magnitudes
with every subtraction an addition: S, the sum of the magnitudes of the terms).  The classes of comparison:

  bits    np.array_equal on the bit patterns (NaN positions included): copies, gathers, masks, max, clamps, one rounding per element,
          the ordered fp32 sums (conv in-diff ascending p, max-pool backward ascending q, splice backward ascending k), the integer scatter
  bound   |got - ref64| <= k * 2^-24 * S element by element; k = the fp32 roundings of the kernel's expression, counted in the source and
          written beside the case (a sum of n terms: n + the epilogue's)
  ulp     library functions: distance in float32 ulps of the float64 result <= LIB_BAR[fn] = max(3 x the worst distance of the numpy-float32
          evaluation of the same expression on the same inputs, 2), and the project's 1e-4 of max(1, |ref|) as a ceiling on top

Every operand is a view into a wider buffer (Operand); `judge` also holds every word outside the view to its initial bits.
"""
import zlib

import numpy as np
from numpy.lib.stride_tricks import as_strided

U = 2.0 ** -24
NAN = np.float32("nan")
SENTINEL = np.float32(-9.87654e17)
MAX_ITEMS = 2048 * 256          # grid_for caps the grid at 2048 blocks of 256: more items than this take a grid-stride iteration
f32, f64 = np.float32, np.float64

# worst float32-ulp distance of the numpy-float32 evaluation over the case tables, per library function, rounded up to two digits, as
# test_substrate_ref_cpu.py measured and prints it (numpy's float32 log / exp are vector routines of a few ulp, not the C library's; that
# file holds what it measures anywhere to twice these); the bar is max(3 x this, 2)
LIB_NUMPY_WORST = {"log": 2.7, "exp": 2.0, "pow": 0.98, "sqrt": 0.5, "sigmoid": 3.5, "tanh": 2.4, "pnorm": 3.1, "pnorm_deriv": 2.1}


def lib_bar(fn):
    return max(3.0 * LIB_NUMPY_WORST[fn], 2.0)


# ---- arithmetic ------------------------------------------------------------------------------------------------------------------------
class F64:
    name, dt = "f64", f64

    def x(self, a): return np.asarray(a, f32).astype(f64)
    def c(self, v): return f64(f32(v))
    def r(self, v): return v
    def mul(self, a, b): return self.r(a * b)
    def add(self, a, b): return self.r(a + b)
    def sub(self, a, b): return self.r(a - b)
    def div(self, a, b):
        with np.errstate(all="ignore"):
            return self.r(a / b)
    def muladd(self, a, b, c): return self.add(self.mul(a, b), c)
    def mulsub(self, c, a, b): return self.sub(c, self.mul(a, b))      # c - a b
    def sqrt(self, a):
        with np.errstate(all="ignore"):
            return self.r(np.sqrt(a))
    def fn(self, f, *a):
        with np.errstate(all="ignore"):
            return self.r(f(*a))


class F32(F64):
    name, dt = "f32", f32

    def x(self, a): return np.asarray(a, f32)
    def c(self, v): return f32(v)
    def r(self, v): return np.asarray(v).astype(f32)


class F32F(F32):
    name = "f32-folded"

    def muladd(self, a, b, c): return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)
    def mulsub(self, c, a, b): return (np.asarray(c, f64) - np.asarray(a, f64) * np.asarray(b, f64)).astype(f32)


class ABS(F64):
    name = "abs"

    def x(self, a): return np.abs(np.asarray(a, f32).astype(f64))
    def c(self, v): return abs(f64(f32(v)))
    def sub(self, a, b): return a + b


ARITH = (F64(), F32(), F32F(), ABS())


def ulp32(x):
    """the float32 ulp at |x| of a float64 x"""
    a = np.abs(np.asarray(x, f64))
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    return np.exp2(np.maximum(e, -126.0) - 23.0)


# tanh_ref forms its result as -1 + q or 1 - q with q in [1, 2]: its error is that of a value of magnitude 1, and an ulp of a result near
# zero says nothing about it.  Its distance is therefore counted in ulps of max(|result|, 1).
ULP_FLOOR = {"tanh": 1.0}


def ulp_dist(got, ref, fn=None):
    g, r = np.asarray(got, f64), np.asarray(ref, f64)
    with np.errstate(invalid="ignore"):
        d = np.abs(g - r) / ulp32(np.maximum(np.abs(r), ULP_FLOOR.get(fn, 0.0)))
    same = (np.isnan(g) & np.isnan(r)) | (g == r)
    return np.where(same, 0.0, np.where(np.isnan(d), np.inf, d))


# ---- operands ----------------------------------------------------------------------------------------------------------------------------
class Operand:
    """[rows x cols] with leading dimension ld inside a wider buffer: 4 + off elements in front, two rows and 8 elements behind; `pad` fills
    everything outside the view (NaN for inputs, SENTINEL for outputs and in-place operands, -1 for index vectors)"""

    def __init__(self, data, ld=None, off=0, pad=NAN):
        data = np.asarray(data)
        if data.ndim == 1:
            data = data[None, :]
        self.dtype = data.dtype
        self.rows, self.cols = data.shape
        self.ld = int(ld) if ld is not None else max(self.cols, 1)
        assert self.ld >= self.cols or self.rows <= 1
        self.off = off
        # inputs carry NaN padding (index vectors -1 or 0): a kernel must leave every word of them alone
        self.is_input = bool(pad in (-1, 0)) if data.dtype.kind == "i" else bool(np.isnan(pad))
        self.start = 4 + off
        self.image = np.full(self.start + (self.rows + 2) * self.ld + 8, pad, self.dtype)
        self.view(self.image)[...] = data

    def view(self, img):
        isz = img.dtype.itemsize
        return as_strided(img[self.start:], (self.rows, self.cols), (self.ld * isz, isz))

    def data(self):
        return self.view(self.image).copy()

    def addr(self, base=0):
        return base + self.start * self.dtype.itemsize


def _bits(a):
    """the bit patterns, every NaN as one pattern (NaN positions count, payloads and signs of a NaN do not)"""
    a = np.ascontiguousarray(a)
    b = a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
    if a.dtype.kind == "f" and np.isnan(a).any():
        b = np.where(np.isnan(a), b.dtype.type(1), b)
    return b


def bits(x): return ("bits", np.asarray(x))
def bound(ref, k, S, u=U): return ("bound", np.asarray(ref, f64), float(k), np.asarray(S, f64), u)
def ulp(ref, fn): return ("ulp", np.asarray(ref, f64), fn)


def judge(op, got_image, expect, what=""):
    """an output buffer as it came back against its expectation -> (failures, (class, fraction of the bar used))"""
    fails = []
    got_image = np.asarray(got_image)
    assert got_image.shape == op.image.shape and got_image.dtype == op.image.dtype
    outside = np.ones(op.image.size, bool)
    op.view(outside)[...] = False
    bad = _bits(got_image)[outside] != _bits(op.image)[outside]
    if bad.any():
        fails.append("%s: %d words outside the view changed (first at buffer index %d)" % (what, int(bad.sum()), int(np.flatnonzero(outside)[bad][0])))
    got = op.view(got_image)
    kind, used = expect[0], 0.0
    if got.size == 0:
        return fails, (kind, 0.0)
    if kind == "bits":
        want = np.asarray(expect[1]).astype(op.dtype).reshape(got.shape)
        ne = _bits(got) != _bits(want)
        if ne.any():
            i = np.unravel_index(int(np.argmax(ne)), ne.shape)
            fails.append("%s: %d of %d elements differ in bits, first at %s: got %r, want %r" % (what, int(ne.sum()), ne.size, i, got[i], want[i]))
            used = np.inf
    elif kind == "bound":
        _, ref, k, S, u = expect
        ref, S = np.broadcast_to(ref, got.shape), np.broadcast_to(S, got.shape)
        with np.errstate(invalid="ignore"):
            err = np.abs(got.astype(f64) - ref)
        err = np.where(got.astype(f64) == ref, 0.0, np.where(np.isnan(err), np.inf, err))      # (inf == inf: a zero row's scale)
        bar = k * u * S
        ok = err <= bar
        if not ok.all():
            i = np.unravel_index(int(np.argmax(err - bar)), err.shape)
            fails.append("%s: %d of %d elements outside %g x 2^%d x S, worst at %s: got %r, float64 %r, off %.3e, bar %.3e"
                         % (what, int((~ok).sum()), ok.size, k, int(np.log2(u)), i, got[i], ref[i], err[i], bar[i]))
        with np.errstate(divide="ignore", invalid="ignore"):
            fr = np.where(bar > 0, err / bar, np.where(err > 0, np.inf, 0.0))
        used = float(fr.max())
    elif kind == "ulp":
        _, ref, fn = expect
        ref = np.broadcast_to(ref, got.shape)
        d = ulp_dist(got, ref, fn)
        bar = lib_bar(fn)
        if not (d <= bar).all():
            i = np.unravel_index(int(np.argmax(d)), d.shape)
            fails.append("%s: %s %d of %d elements beyond %.2f ulp, worst at %s: got %r, float64 %r, %.2f ulp" % (what, fn, int((d > bar).sum()), d.size, bar, i, got[i], ref[i], d[i]))
        with np.errstate(invalid="ignore"):
            rel = np.abs(got.astype(f64) - ref) / np.maximum(1.0, np.abs(ref))
        rel = np.where(ulp_dist(got, ref) == 0, 0.0, np.where(np.isnan(rel), np.inf, rel))
        if not (rel <= 1e-4).all():
            fails.append("%s: %s %.3e of max(1, |ref|) from float64, above the project's 1e-4" % (what, fn, rel.max()))
        used = float(d.max())
    else:
        raise ValueError(kind)
    return fails, (kind if kind != "ulp" else "ulp:" + expect[2], used)


class Case:
    """ops: name -> Operand in the order the entry point takes them; par: scalars; expect: output name -> expectation; evals: fp32
    evaluations [{output name: array}]; path: what the host's predicate must pick"""

    def __init__(self, op, name, ops, par=None, expect=None, evals=None, path=None, k=""):
        self.op, self.name, self.ops, self.par, self.expect, self.evals, self.path, self.k = op, name, ops, par or {}, expect or {}, evals or [], path, k
        self.deriv = None

    @property
    def id(self):
        return "%s-%s" % (self.op, self.name)


def rng_of(*key):
    """a generator seeded by the case's own key: every case draws the same inputs wherever and in whatever order it is built"""
    return np.random.default_rng(zlib.crc32("|".join(str(k) for k in key).encode()))


def vec_path(cols, ops):
    """the predicate of launch_map / launch_row_gather / splice / add_row_sum_mat on (address, ld) pairs: 16-byte accesses when cols % 4 == 0, every
    stride % 4 == 0 and every base 16-byte aligned"""
    return cols % 4 == 0 and all(ld % 4 == 0 and addr % 16 == 0 for addr, ld in ops)


def path_name(vec, items):
    return ("vec4" if vec else "scalar") + ("-gs" if items > MAX_ITEMS else "")


# ---- launch_map operations ---------------------------------------------------------------------------------------------------------------
# (rows, cols, pitch, offset) of the issue's access-path grid; the last two reach a grid-stride iteration
GRID = [(1, 1, 1, 0), (37, 53, 53, 0), (5, 8, 8, 0), (33, 64, 72, 0), (33, 64, 67, 0), (33, 64, 72, 1), (1030, 2048, 2048, 0), (1030, 511, 511, 0)]
GRID_SMALL, GRID_BIG = GRID[:6], GRID[6:]
SRC_MISALIGNED = (33, 64, 72, 0, "src+1")       # only a source operand 4 bytes off: scalar
EMPTY = [(0, 8, 8, 0), (5, 0, 8, 0)]


def _sig(A, x):
    e = A.fn(np.exp, -np.abs(x))
    return A.div(np.where(x > 0, A.dt(1), e), A.add(A.dt(1), e))


def _tanh(A, x):
    ie = A.fn(np.exp, -np.abs(x))
    q = A.div(A.dt(2), A.muladd(ie, ie, A.dt(1)))
    return np.where(x > 0, A.add(A.dt(-1), q), A.sub(A.dt(1), q))


def _pow(A, d, p):
    if p == 1.0: return d
    if p == 2.0: return A.mul(d, d)
    if p == 0.5: return A.sqrt(d)
    return A.fn(np.power, d, A.dt(f32(p)))


# name -> (reads dst, sources, vector ('row': indexed by the column, 'col': by the row), f(A, d, a, b, v, p), class, parameters, input domain)
# class: "bits", ("ulp", fn) or the count k of fp32 roundings in the functor
MAP_OPS = {
    "set_const": (False, 0, None, lambda A, d, a, b, v, p: np.full(d.shape, A.c(p["v"])), "bits", dict(v=-2.625), "n"),
    "add": (True, 0, None, lambda A, d, a, b, v, p: A.add(d, A.c(p["v"])), "bits", dict(v=0.37), "n"),
    "scale": (True, 0, None, lambda A, d, a, b, v, p: A.mul(d, A.c(p["v"])), "bits", dict(v=-1.7), "n"),
    "apply_log": (True, 0, None, lambda A, d, a, b, v, p: A.fn(np.log, d), ("ulp", "log"), {}, "pos"),
    "apply_exp": (True, 0, None, lambda A, d, a, b, v, p: A.fn(np.exp, d), ("ulp", "exp"), {}, "n"),
    "apply_pow2": (True, 0, None, lambda A, d, a, b, v, p: _pow(A, d, 2.0), "bits", dict(v=2.0), "n"),
    "apply_pow1": (True, 0, None, lambda A, d, a, b, v, p: _pow(A, d, 1.0), "bits", dict(v=1.0), "n"),
    "apply_pow_half": (True, 0, None, lambda A, d, a, b, v, p: _pow(A, d, 0.5), ("ulp", "sqrt"), dict(v=0.5), "pos"),
    "apply_pow": (True, 0, None, lambda A, d, a, b, v, p: _pow(A, d, 1.7), ("ulp", "pow"), dict(v=1.7), "pos"),
    "apply_heaviside": (True, 0, None, lambda A, d, a, b, v, p: np.where(d > 0, A.dt(1), A.dt(0)), "bits", {}, "edge0"),
    "apply_clamp": (True, 0, None, lambda A, d, a, b, v, p: np.where(d < A.c(p["lo"]), A.c(p["lo"]), np.where(d > A.c(p["hi"]), A.c(p["hi"]), d)), "bits", dict(lo=-0.5, hi=0.75), "edge"),
    "apply_floor": (True, 0, None, lambda A, d, a, b, v, p: np.where(d < A.c(p["v"]), A.c(p["v"]), d), "bits", dict(v=-0.5), "edge"),
    "apply_ceiling": (True, 0, None, lambda A, d, a, b, v, p: np.where(d > A.c(p["v"]), A.c(p["v"]), d), "bits", dict(v=0.75), "edge"),
    "invert_elements": (True, 0, None, lambda A, d, a, b, v, p: A.div(A.dt(1), d), 1, {}, "pos"),                      # 1 / d: one rounding
    "mul_elements": (True, 1, None, lambda A, d, a, b, v, p: A.mul(d, a), "bits", {}, "n"),
    "mul_cols_vec": (True, 0, "row", lambda A, d, a, b, v, p: A.mul(d, v), "bits", {}, "n"),
    "mul_rows_vec": (True, 0, "col", lambda A, d, a, b, v, p: A.mul(d, v), "bits", {}, "n"),
    "add_mat": (True, 1, None, lambda A, d, a, b, v, p: A.muladd(A.c(p["alpha"]), a, d), 2, dict(alpha=-0.75), "n"),   # alpha a, + d
    "add_vec_to_cols": (True, 0, "col", lambda A, d, a, b, v, p: A.muladd(A.c(p["alpha"]), v, A.mul(A.c(p["beta"]), d)), 3, dict(alpha=-1.5, beta=0.5), "n"),
    "add_vec_to_rows": (True, 0, "row", lambda A, d, a, b, v, p: A.muladd(A.c(p["alpha"]), v, A.mul(A.c(p["beta"]), d)), 3, dict(alpha=0.5, beta=-0.25), "n"),
    "add_vec_to_rows_beta0": (False, 0, "row", lambda A, d, a, b, v, p: A.mul(A.c(p["alpha"]), v) + np.zeros(d.shape, A.dt), "bits", dict(alpha=0.5, beta=0.0), "n"),
    "add_mat_diag_vec": (True, 1, "row", lambda A, d, a, b, v, p: A.muladd(A.mul(A.c(p["alpha"]), a), v, A.mul(A.c(p["beta"]), d)), 4, dict(alpha=0.75, beta=-0.5), "n"),
    "add_mat_mat_elements": (True, 2, None, lambda A, d, a, b, v, p: A.muladd(A.mul(A.c(p["alpha"]), a), b, A.mul(A.c(p["beta"]), d)), 4, dict(alpha=-1.25, beta=0.5), "n"),
    "add_mat_mat_elements_beta0": (False, 2, None, lambda A, d, a, b, v, p: A.mul(A.mul(A.c(p["alpha"]), a), b), 2, dict(alpha=-1.25, beta=0.0), "n"),
    "sigmoid": (False, 1, None, lambda A, d, a, b, v, p: _sig(A, a), ("ulp", "sigmoid"), {}, "wide"),
    "tanh": (False, 1, None, lambda A, d, a, b, v, p: _tanh(A, a), ("ulp", "tanh"), {}, "wide"),
    "diff_sigmoid": (False, 2, None, lambda A, d, a, b, v, p: A.mul(A.mul(a, b), A.sub(A.dt(1), b)), 3, {}, "unit"),          # e y, 1 - y, product
    "diff_tanh": (False, 2, None, lambda A, d, a, b, v, p: A.mul(a, A.mulsub(A.dt(1), b, b)), 3, {}, "unit"),               # y y, 1 - ., e .
    "diff_relu": (False, 2, None, lambda A, d, a, b, v, p: np.where(a > 0, b, A.dt(0)), "bits", {}, "edge0"),
    "copy_mat": (False, 1, None, lambda A, d, a, b, v, p: a, "bits", {}, "n"),
}
UNARY_INPLACE = [n for n, s in MAP_OPS.items() if s[0] and s[1] == 0]
BIG_UNARY = ("mul_cols_vec", "scale")


def _draw(rng, shape, domain):
    x = rng.standard_normal(shape).astype(f32)
    if domain == "pos": x = (np.abs(x) * f32(1.5) + f32(0.05)).astype(f32)
    elif domain == "wide": x = (x * f32(4)).astype(f32)
    elif domain == "unit": x = (f32(0.5) + f32(0.45) * np.tanh(x)).astype(f32)
    elif domain in ("edge", "edge0") and x.size:
        flat = x.reshape(-1)
        for i, val in enumerate((0.0, -0.0, -0.5, 0.75) if domain == "edge" else (0.0, -0.0, 1e-30, -1e-30)):
            flat[(7 * i + 3) % flat.size if flat.size > 4 else i % flat.size] = val
    return x


def evaluate(model, inputs, k):
    """a model under the four arithmetics -> (expectation class pieces, fp32 evaluations)"""
    r64, r32, r32f, S = (model(A, *[A.x(i) if i is not None else None for i in inputs]) for A in ARITH)
    if k == "bits":
        assert np.array_equal(_bits(np.asarray(r32, f32)), _bits(np.asarray(r32f, f32)))
        return bits(np.asarray(r32, f32)), [r32, r32f]
    if isinstance(k, tuple):
        return ulp(r64, k[1]), [r32, r32f]
    return bound(r64, k, S), [r32, r32f]


def map_case(opname, rows, cols, pitch, off, src_off=0):
    read_dst, nsrc, vk, f, k, par, domain = MAP_OPS[opname]
    rng = rng_of(opname, rows, cols, pitch, off)
    d0 = _draw(rng, (rows, cols), domain) if read_dst else np.full((rows, cols), NAN, f32)
    srcs = [_draw(rng, (rows, cols), domain) for _ in range(nsrc)]
    if opname == "diff_sigmoid": srcs[0] = _draw(rng, (rows, cols), "n")
    if opname == "diff_tanh": srcs = [_draw(rng, (rows, cols), "n"), (2 * srcs[1] - 1).astype(f32)]
    if opname == "diff_relu": srcs[1] = _draw(rng, (rows, cols), "n")
    v = _draw(rng, (cols if vk == "row" else rows,), "n") if vk else None
    vb = None if v is None else (v[None, :] if vk == "row" else v[:, None])
    a, b = (srcs + [None, None])[:2]
    ops = {"dst": Operand(d0, pitch, off, SENTINEL)}
    for nm, s in zip("ab", srcs):
        ops[nm] = Operand(s, pitch + (4 if nm == "b" and pitch % 4 == 0 and pitch > cols else 0), off + src_off, NAN)
    if v is not None:
        ops["v"] = Operand(v, None, 0, NAN)
    model = lambda A, d, a, b, v: f(A, d, a, b, v, par)
    exp, evals = evaluate(model, (d0, a, b, vb), k)
    vec = vec_path(cols, [(o.addr(), o.ld) for n, o in ops.items() if n != "v"])
    items = rows * (cols // 4 if vec else cols)
    name = "%dx%d-ld%d%s%s" % (rows, cols, pitch, "-off%d" % off if off else "", "-src+%d" % src_off if src_off else "")
    return Case(opname, name, ops, par, {"dst": exp}, [{"dst": e} for e in evals], path_name(vec, items), k)


def map_table():
    """(id, builder) of every launch_map case"""
    t = []
    for opname in MAP_OPS:
        shapes = list(GRID_SMALL)
        if opname not in UNARY_INPLACE or opname in BIG_UNARY:
            shapes += GRID_BIG
        for s in shapes:
            t.append((opname, s, 0))
        if MAP_OPS[opname][1] > 0:
            t.append((opname, SRC_MISALIGNED[:4], 1))
        for s in EMPTY:
            t.append((opname, s, 0))
    return [("%s-%dx%d-ld%d-off%d%s" % (o, s[0], s[1], s[2], s[3], "-src+1" if so else ""), (lambda o=o, s=s, so=so: map_case(o, *s, src_off=so))) for o, s, so in t]


# ---- the other kernels of ew_kernels.hip ---------------------------------------------------------------------------------------------------
def add_mat_trans_case():
    """37 x 53 += alpha * (pitched 53 x 37)^T; k = 2: alpha s, + d"""
    rng = rng_of("add_mat_trans")
    d0, s, alpha = _draw(rng, (37, 53), "n"), _draw(rng, (53, 37), "n"), -0.75
    exp, evals = evaluate(lambda A, d, s: A.muladd(A.c(alpha), s.T, d), (d0, s), 2)
    return Case("add_mat_trans", "37x53", {"dst": Operand(d0, 56, 1, SENTINEL), "src": Operand(s, 41, 0, NAN)}, dict(alpha=alpha), {"dst": exp}, [{"dst": e} for e in evals], "trans", 2)


def add_mat_diag_vec_strided_case():
    """mat2 read transposed (row stride 1, column stride the pitch of the stored 53 x 37); k = 4"""
    rng = rng_of("mdv_strided")
    d0, mt, v, alpha, beta = _draw(rng, (37, 53), "n"), _draw(rng, (53, 37), "n"), _draw(rng, (53,), "n"), -0.5, 0.75
    exp, evals = evaluate(lambda A, d, m, v: A.muladd(A.mul(A.c(alpha), m.T), v, A.mul(A.c(beta), d)), (d0, mt, v[None, :]), 4)
    return Case("add_mat_diag_vec_strided", "37x53", {"dst": Operand(d0, 55, 0, SENTINEL), "m2": Operand(mt, 39, 0, NAN), "v": Operand(v)}, dict(alpha=alpha, beta=beta),
                {"dst": exp}, [{"dst": e} for e in evals], "strided", 4)


def regularize_l1_model(w, g, l1, lr):
    """cu-kernels.cu _regularize_l1 in float32; -> (w, grad, |after| so the caller can keep the sign test away from a rounding)"""
    l1, lr = f32(l1), f32(lr)
    l1s = np.where(w < 0, -l1, l1).astype(f32)
    after = (w.astype(f64) - lr.astype(f64) * g - l1s)
    flip = (after > 0) ^ (w > 0)
    zero = w == 0
    wo = np.where(zero, w, np.where(flip, f32(0), (w - l1s).astype(f32))).astype(f32)
    go = np.where(~zero & flip, f32(0), g).astype(f32)
    return wo, go, np.where(zero, np.inf, np.abs(after))


def regularize_l1_case(rows=37, cols=53):
    rng = rng_of("l1", rows, cols)
    w, g = (_draw(rng, (rows, cols), "n") * f32(0.01)).astype(f32), _draw(rng, (rows, cols), "n")
    w[rng.random((rows, cols)) < 0.1] = 0
    l1, lr = 0.002, 0.01
    for _ in range(8):      # keep the sign test away from zero by more than any rounding of `after`
        near = regularize_l1_model(w, g, l1, lr)[2] < 1e-6
        w[near] = (w[near] * f32(1.5) + f32(1e-4)).astype(f32)
    wo, go, margin = regularize_l1_model(w, g, l1, lr)
    assert margin.min() >= 1e-6 and (wo == 0).sum() > (w == 0).sum() and ((wo != 0) & (w != 0)).any()
    return Case("regularize_l1", "%dx%d" % (rows, cols), {"w": Operand(w, cols + 3, 0, SENTINEL), "g": Operand(g, cols + 6, 1, SENTINEL)}, dict(l1=l1, lr=lr),
                {"w": bits(wo), "g": bits(go)}, [{"w": wo, "g": go}], "l1", "bits")


def row_gather_case(opname, rows, cols, pitch, off, src_off=0):
    """copy_rows / randomize: dst[r] = src[idx[r]] (idx < 0: zeros); add_rows: dst[r] += alpha src[idx[r]], k = 2"""
    rng = rng_of(opname, rows, cols, pitch, off)
    nsrc = max(rows // 2 + 3, 1)
    src = _draw(rng, (nsrc, cols), "n")
    idx = rng.integers(0, nsrc, rows).astype(np.int32)
    if rows > 3:
        idx[1], idx[2], idx[rows - 1] = -1, idx[0], -1
    d0 = _draw(rng, (rows, cols), "n") if opname == "add_rows" else np.full((rows, cols), NAN, f32)
    g = np.where(idx[:, None] < 0, f32(0), src[np.maximum(idx, 0)]) if rows else np.zeros((0, cols), f32)
    alpha = 0.625 if opname == "add_rows" else 0.0
    if opname == "add_rows":
        exp, evals = evaluate(lambda A, d, g: A.muladd(A.c(alpha), g, d), (d0, g), 2)
    else:
        exp, evals = bits(g), [g, g]
    ops = {"dst": Operand(d0, pitch, off, SENTINEL), "src": Operand(src, pitch + (8 if pitch % 4 == 0 and pitch > cols else 0), off + src_off, NAN), "idx": Operand(idx, None, 0, -1)}
    vec = vec_path(cols, [(ops["dst"].addr(), ops["dst"].ld), (ops["src"].addr(), ops["src"].ld)])
    name = "%dx%d-ld%d%s%s" % (rows, cols, pitch, "-off%d" % off if off else "", "-src+%d" % src_off if src_off else "")
    return Case(opname, name, ops, dict(alpha=alpha), {"dst": exp}, [{"dst": e} for e in evals], path_name(vec, rows * (cols // 4 if vec else cols)), 2 if opname == "add_rows" else "bits")


def row_gather_table():
    t = []
    for o in ("copy_rows", "add_rows", "randomize"):
        for s in GRID + EMPTY:
            t.append((o, s, 0))
        t.append((o, SRC_MISALIGNED[:4], 1))
    return [("%s-%dx%d-ld%d-off%d%s" % (o, s[0], s[1], s[2], s[3], "-src+1" if so else ""), (lambda o=o, s=s, so=so: row_gather_case(o, *s, src_off=so))) for o, s, so in t]


def col_gather_case(opname, rows=29, cols=9, src_cols=17):
    """copy_cols / copy: dst[r][c] = src[r][reorder[c]] (< 0: zero); add_cols: dst += (one rounding); the source is wider than the destination"""
    rng = rng_of(opname, rows, cols)
    src = _draw(rng, (rows, src_cols), "n")
    idx = rng.integers(0, src_cols, cols).astype(np.int32)
    idx[1], idx[3], idx[cols - 1] = -1, idx[0], src_cols - 1
    d0 = _draw(rng, (rows, cols), "n") if opname == "add_cols" else np.full((rows, cols), NAN, f32)
    g = np.where(idx[None, :] < 0, f32(0), src[:, np.maximum(idx, 0)])
    out = (d0 + g).astype(f32) if opname == "add_cols" else g
    return Case(opname, "%dx%d-from-%d" % (rows, cols, src_cols), {"dst": Operand(d0, cols + 3, 1, SENTINEL), "src": Operand(src, src_cols + 5, 0, NAN), "idx": Operand(idx, None, 0, -1)},
                {}, {"dst": bits(out)}, [{"dst": out}], "cols", "bits")


def splice_model(x, offs):
    rows = x.shape[0]
    return np.concatenate([x[np.clip(np.arange(rows) + o, 0, rows - 1)] for o in offs], axis=1)


def splice_bwd_model(od, offs, in_cols, dt=f32):
    """ascending k from a zero accumulator, in dt"""
    rows = od.shape[0]
    acc = np.zeros((rows, in_cols), dt)
    for k, o in enumerate(offs):
        acc = (acc + od[np.clip(np.arange(rows) + o, 0, rows - 1), k * in_cols:(k + 1) * in_cols].astype(dt)).astype(dt)
    return acc


SPLICE = [(8, 12, 60, 0), (40, 44, 284, 0), (13, 16, 94, 0), (8, 12, 58, 0), (8, 12, 60, 1)]   # in_cols, ldx, ldy, offset: vec, vec, scalar x 3
SPLICE_OFFS = np.array([-31, -2, -1, 0, 1, 3, 40], np.int32)                                     # beyond both ends of 29 rows


def splice_case(back, in_cols, ldx, ldy, off, rows=29):
    rng = rng_of("splice", back, in_cols, ldx, ldy, off)
    n_off = len(SPLICE_OFFS)
    name = "%dx%d-ldx%d-ldy%d%s" % (rows, in_cols, ldx, ldy, "-off1" if off else "")
    if not back:
        x = _draw(rng, (rows, in_cols), "n")
        y = splice_model(x, SPLICE_OFFS)
        ops = {"y": Operand(np.full(y.shape, NAN, f32), ldy, off, SENTINEL), "x": Operand(x, ldx, 0, NAN), "off": Operand(SPLICE_OFFS, None, 0, 0)}
        vec = in_cols % 4 == 0 and ldx % 4 == 0 and ldy % 4 == 0 and ops["y"].addr() % 16 == 0 and ops["x"].addr() % 16 == 0
        return Case("splice", name, ops, {}, {"y": bits(y)}, [{"y": y}], path_name(vec, 0), "bits")
    od = _draw(rng, (rows, in_cols * n_off), "n")
    idf = splice_bwd_model(od, SPLICE_OFFS, in_cols)
    ops = {"in_diff": Operand(np.full(idf.shape, NAN, f32), ldx, off, SENTINEL), "od": Operand(od, ldy, 0, NAN), "off": Operand(SPLICE_OFFS, None, 0, 0)}
    vec = in_cols % 4 == 0 and ldx % 4 == 0 and ldy % 4 == 0 and ops["in_diff"].addr() % 16 == 0 and ops["od"].addr() % 16 == 0
    return Case("splice_backward", name, ops, dict(n_off=n_off), {"in_diff": bits(idf)}, [{"in_diff": idf}], path_name(vec, 0), "bits")


def set_const_i32_case():
    d0 = np.arange(7 * 11, dtype=np.int32).reshape(7, 11)
    return Case("set_const_i32", "7x11-ld14", {"dst": Operand(d0, 14, 1, np.int32(-77))}, dict(v=123456789), {"dst": bits(np.full((7, 11), 123456789, np.int32))},
                [{"dst": np.full((7, 11), 123456789, np.int32)}], "i32", "bits")


VEC_N = [1, 255, 256, 257, 524325]


def scatter_add_case(n=524288 + 37, rows=19, cols=23):
    """small-integer values: every partial sum is an exact float32, so any atomic order gives these bits"""
    rng = rng_of("scatter", n)
    r, c = rng.integers(-2, rows + 2, n).astype(np.int32), rng.integers(-2, cols + 2, n).astype(np.int32)
    vals = rng.integers(-3, 4, n).astype(f32)
    d0 = rng.integers(-5, 6, (rows, cols)).astype(f32)
    ok = (r >= 0) & (r < rows) & (c >= 0) & (c < cols)
    out = d0.astype(f64)
    np.add.at(out, (r[ok], c[ok]), vals[ok].astype(f64))
    assert np.abs(out).max() < 2 ** 23 and (~ok).sum() > 0
    return Case("scatter_add", "n%d" % n, {"dst": Operand(d0, cols + 2, 1, SENTINEL), "rows": Operand(r, None, 0, -1), "cols": Operand(c, None, 0, -1), "vals": Operand(vals)},
                dict(n=n), {"dst": bits(out.astype(f32))}, [{"dst": out.astype(f32)}], "scatter", "bits")


def f2d_case(n):
    x = _draw(rng_of("f2d", n), (n,), "n")
    return Case("f2d", "n%d" % n, {"dst": Operand(np.full(n, np.nan, f64), None, 0, f64(SENTINEL)), "src": Operand(x, None, 1, NAN)}, dict(n=n), {"dst": bits(x.astype(f64))},
                [{"dst": x.astype(f64)}], "vec", "bits")


def d2f_case(n):
    """round to nearest even: values just above, just below and exactly at the middle of two neighbouring float32"""
    rng = rng_of("d2f", n)
    base = _draw(rng, (n,), "n").astype(f64)
    half = np.spacing(base.astype(f32)).astype(f64) / 2
    x = base + half * rng.choice(np.array([0.0, 1.0, -1.0, 0.999, -0.999, 1.001, -1.001, 0.3]), n)
    return Case("d2f", "n%d" % n, {"dst": Operand(np.full(n, NAN, f32), None, 1, SENTINEL), "src": Operand(x, None, 0, f64("nan"))}, dict(n=n), {"dst": bits(x.astype(f32))},
                [{"dst": x.astype(f32)}], "vec", "bits")


def vec_case(opname, n):
    """add_vec_vec: alpha x y + beta v, k = 4; vec_axpy(2): y += alpha x, k = 2; vec_diff: a - b, one rounding"""
    rng = rng_of(opname, n)
    x, y, v, x2, y2 = (_draw(rng, (n,), "n") for _ in range(5))
    mk = lambda arr, off=0, out=False: Operand(arr, None, off, SENTINEL if out else NAN)
    if opname == "add_vec_vec":
        al, be = 0.75, -0.5
        exp, ev = evaluate(lambda A, v, x, y: A.muladd(A.mul(A.c(al), x), y, A.mul(A.c(be), v)), (v, x, y), 4)
        return Case(opname, "n%d" % n, {"v": mk(v, 1, True), "x": mk(x), "y": mk(y, 1)}, dict(alpha=al, beta=be, n=n), {"v": exp}, [{"v": e} for e in ev], "vec", 4)
    if opname == "vec_axpy":
        exp, ev = evaluate(lambda A, y, x: A.muladd(A.c(-0.3), x, y), (y, x), 2)
        return Case(opname, "n%d" % n, {"x": mk(x, 1), "y": mk(y, 0, True)}, dict(alpha=-0.3, n=n), {"y": exp}, [{"y": e} for e in ev], "vec", 2)
    if opname == "vec_axpy2":
        e1, ev1 = evaluate(lambda A, y, x: A.muladd(A.c(-0.3), x, y), (y, x), 2)
        e2, ev2 = evaluate(lambda A, y, x: A.muladd(A.c(-0.3), x, y), (y2, x2), 2)
        return Case(opname, "n%d" % n, {"x1": mk(x), "y1": mk(y, 1, True), "x2": mk(x2, 1), "y2": mk(y2, 0, True)}, dict(alpha=-0.3, n=n), {"y1": e1, "y2": e2},
                    [{"y1": a, "y2": b} for a, b in zip(ev1, ev2)], "vec", 2)
    out = (x - y).astype(f32)
    return Case("vec_diff", "n%d" % n, {"out": mk(np.full(n, NAN, f32), 1, True), "a": mk(x), "b": mk(y, 1)}, dict(n=n), {"out": bits(out)}, [{"out": out}], "vec", "bits")


def dropout_uniform(seed, n):
    """splitmix64 of (seed, element index) -> 24 bits in [0, 1), as dropout_uniform in csrc/ew_kernels.hip"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (np.arange(n, dtype=np.uint64) + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(f32) * f32(1.0 / 16777216.0)


def dropout_case(rows, cols, retention, seed, pitched):
    rng = rng_of("dropout", rows, cols)
    x, od = _draw(rng, (rows, cols), "n"), _draw(rng, (rows, cols), "n")
    mask = (dropout_uniform(seed, rows * cols) < f32(retention)).astype(f32).reshape(rows, cols)
    inv = f32(1.0) / f32(retention)
    out, idf = ((x * mask).astype(f32) * inv).astype(f32), ((od * mask).astype(f32) * inv).astype(f32)
    p = (lambda c, k: c + k) if pitched else (lambda c, k: c)
    nan = np.full((rows, cols), NAN, f32)
    ops = {"out": Operand(nan, p(cols, 3), int(pitched), SENTINEL), "in": Operand(x, p(cols, 5), 0, NAN), "mask": Operand(nan, p(cols, 1), 0, SENTINEL),
           "in_diff": Operand(nan, p(cols, 2), 0, SENTINEL), "od": Operand(od, p(cols, 7), int(pitched), NAN)}
    return Case("dropout", "%dx%d-r%g-s%d%s" % (rows, cols, retention, seed, "-pitched" if pitched else ""), ops, dict(retention=retention, seed=seed),
                {"out": bits(out), "mask": bits(mask), "in_diff": bits(idf)}, [{"out": out, "mask": mask, "in_diff": idf}], "dropout", "bits")


DROPOUT = [(7, 13, 0.5, 11, True), (7, 13, 0.5, 11, False), (7, 13, 0.5, 12, True), (5, 9, 1.0, 3, True), (256, 512, 0.3, 5, False), (256, 512, 0.8, 5, True)]


# ---- conv_pool.hip -----------------------------------------------------------------------------------------------------------------------
CONV = [(3, 4, 1, 10, 7, 3), (2, 3, 3, 9, 3, 3), (1, 2, 3, 11, 4, 3), (2, 3, 2, 10, 3, 3), (1, 5, 1, 5, 1, 3), (11, 9, 1, 40, 32, 3)]   # num_splice, patch_dim, step, stride, P, N
CONV_GS_GATHER, CONV_GS_INDIFF = (11, 9, 1, 40, 32, 170), (11, 9, 1, 40, 32, 1200)


def conv_gather_model(x, ns, pd, step, stride, P):
    N = x.shape[0]
    out = np.empty((N * P, ns * pd), x.dtype)
    for p in range(P):
        for s in range(ns):
            out[p::P, s * pd:(s + 1) * pd] = x[:, p * step + s * stride: p * step + s * stride + pd]
    return out


def conv_indiff_model(pdiff, ns, pd, step, stride, P, dt=f32):
    """ascending p from a zero accumulator in dt; columns no patch covers stay exactly 0"""
    N = pdiff.shape[0] // P
    acc = np.zeros((N, ns * stride), dt)
    for p in range(P):
        for s in range(ns):
            sl = slice(s * stride + p * step, s * stride + p * step + pd)
            acc[:, sl] = (acc[:, sl] + pdiff[p::P, s * pd:(s + 1) * pd].astype(dt)).astype(dt)
    return acc


def conv_case(back, ns, pd, step, stride, P, N):
    rng = rng_of("conv", back, ns, pd, step, stride, P, N)
    fd, name = ns * pd, "s%d-d%d-st%d-str%d-P%d-N%d" % (ns, pd, step, stride, P, N)
    geo = dict(P=P, ns=ns, pd=pd, step=step, stride=stride)
    if not back:
        x = _draw(rng, (N, ns * stride + 3), "n")       # wider than num_splice * stride
        out = conv_gather_model(x, ns, pd, step, stride, P)
        ops = {"patches": Operand(np.full(out.shape, NAN, f32), fd + 5, 1, SENTINEL), "in": Operand(x, x.shape[1] + 2, 0, NAN)}
        return Case("conv_gather", name, ops, geo, {"patches": bits(out)}, [{"patches": out}], "gs" if out.size > MAX_ITEMS else "one", "bits")
    pdiff = (_draw(rng, (N * P, fd), "n") + f32(0.5)).astype(f32)
    out = conv_indiff_model(pdiff, ns, pd, step, stride, P)
    ops = {"in_diff": Operand(np.full(out.shape, NAN, f32), ns * stride + 3, 1, SENTINEL), "patch_diff": Operand(pdiff, fd + 5, 0, NAN)}
    return Case("conv_in_diff", name, ops, geo, {"in_diff": bits(out)}, [{"in_diff": out}], "gs" if out.size > MAX_ITEMS else "one", "bits")


POOL = [(14, 3, 1, 3), (32, 4, 4, 128), (11, 2, 3, 4), (10, 3, 2, 1), (6, 6, 1, 5)]     # num_patches, size, step, stride


def maxpool_fwd_model(x, size, step, stride):
    npatch = x.shape[1] // stride
    npool = 1 + (npatch - size) // step
    out = np.full((x.shape[0], npool * stride), f32(-1e20), f32)
    for q in range(npool):
        for r in range(size):
            out[:, q * stride:(q + 1) * stride] = np.fmax(out[:, q * stride:(q + 1) * stride], x[:, (q * step + r) * stride:(q * step + r + 1) * stride])
    return out


def maxpool_bwd_model(x, out, od, size, step, stride, dt=f32):
    """ascending q from a zero accumulator, then times (float)(1.0 / summands); a patch no pool covers: exactly 0"""
    npatch, npool = x.shape[1] // stride, out.shape[1] // stride
    acc, cnt = np.zeros(x.shape, dt), np.zeros(npatch, int)
    for q in range(npool):
        for r in range(size):
            p = q * step + r
            sl, ql = slice(p * stride, (p + 1) * stride), slice(q * stride, (q + 1) * stride)
            mask = (x[:, sl] == out[:, ql]).astype(dt)
            acc[:, sl] = (acc[:, sl] + (od[:, ql].astype(dt) * mask).astype(dt)).astype(dt)
            cnt[p] += 1
    scale = np.array([dt(1.0 / c) if c else dt(0) for c in cnt], dt)
    return (acc * np.repeat(scale, stride)[None, :]).astype(dt), cnt


def maxpool_case(npatch, size, step, stride, N=7):
    rng = rng_of("pool", npatch, size, step, stride)
    x = rng.choice(np.array([-1.5, -0.25, 0.0, 0.5, 2.0], f32), (N, npatch * stride)).astype(f32)      # five values: pools tie
    x[1, :] = f32(0.5)
    x[2, :] = rng.choice(np.array([-1e20, -3e20, -np.inf], f32), npatch * stride)
    x[3, ::2] = f32(-2e20)
    out = maxpool_fwd_model(x, size, step, stride)
    assert (out[2] == f32(-1e20)).all()
    od = (_draw(rng, out.shape, "n") + f32(0.5)).astype(f32)
    idf, cnt = maxpool_bwd_model(x, out, od, size, step, stride)
    ops = {"out": Operand(np.full(out.shape, NAN, f32), out.shape[1] + 3, 1, SENTINEL), "in": Operand(x, x.shape[1] + 2, 0, NAN),
           "in_diff": Operand(np.full(x.shape, NAN, f32), x.shape[1] + 1, 0, SENTINEL), "od": Operand(od, out.shape[1] + 6, 1, NAN)}
    return Case("max_pool", "p%d-sz%d-st%d-str%d" % (npatch, size, step, stride), ops, dict(size=size, step=step, stride=stride), {"out": bits(out), "in_diff": bits(idf)},
                [{"out": out, "in_diff": idf}], "uncovered" if (cnt == 0).any() else "covered", "bits")


LN_D, LN_N = [1, 5, 40, 64, 65, 100, 1000], [1, 3, 4, 5, 9]
LN_CASES = [(n, d) for d in LN_D for n in LN_N] + [(8200, 8)]


def length_norm_out(x, scale32):
    """out == fl(x * scale) from the float32 scales as returned (a zero row: scale inf, 0 * inf = NaN, as the reference's sequence gives)"""
    with np.errstate(all="ignore"):
        return (x * np.asarray(scale32, f32)[:, None]).astype(f32)


def length_norm_scales(A, x):
    """1 / sqrt(sum fl(x * x)): the squares are float32 in the reference (l2_aux_ is a float matrix), the sum is in double.  k = 3: the sum to float,
    sqrtf, the division"""
    sq = (np.asarray(x, f32) * np.asarray(x, f32)).astype(f32).astype(f64).sum(axis=1)
    if A.name == "abs": return 1.0 / np.sqrt(np.where(sq > 0, sq, 1.0))
    if A.dt is f64:
        with np.errstate(all="ignore"):
            return 1.0 / np.sqrt(sq)
    with np.errstate(all="ignore"):
        return (f32(1) / np.sqrt(sq.astype(f32)).astype(f32)).astype(f32)


def length_norm_case(N, D):
    x = _draw(rng_of("ln", N, D), (N, D), "n")
    if N >= 3: x[1, :] = 0
    with np.errstate(all="ignore"):
        sc64, sc32, S = length_norm_scales(ARITH[0], x), length_norm_scales(ARITH[1], x), length_norm_scales(ARITH[3], x)
    zero = ~np.isfinite(sc64)
    # the zero row through the reference's own op sequence in float32: sum 0, sqrt 0, 1 / 0 = inf; the model above gives exactly that
    exp = bound(np.where(zero, np.inf, sc64), 3, np.where(zero, 0.0, S))
    ops = {"out": Operand(np.full((N, D), NAN, f32), D + 3, 1, SENTINEL), "in": Operand(x, D + 2, 0, NAN), "scales": Operand(np.full(N, NAN, f32), None, 1, SENTINEL)}
    return Case("length_norm", "%dx%d" % (N, D), ops, {}, {"scales": exp}, [{"scales": sc32}], "gs" if N > 2048 * 4 else "one", 3)


GROUPS, POWERS = [1, 2, 5, 10], [0.0, 1.0, 2.0, 3.0, 1.5]


def group_pnorm_model(A, x, g, p):
    """kaldi-vector.cc Norm(p) per group, the terms added in ascending k; the overflow branch rescales by the largest magnitude"""
    N = x.shape[0]
    xg = x.reshape(N, -1, g)
    one = A.dt(1)
    def seq(terms):
        s = np.zeros(terms.shape[:2], A.dt)
        for k in range(g): s = A.add(s, terms[:, :, k])
        return s
    if p == 0.0: return seq((xg != 0).astype(A.dt))
    if p == 1.0: return seq(np.abs(xg))
    if p == 2.0:
        s = np.zeros(xg.shape[:2], A.dt)
        for k in range(g): s = A.muladd(xg[:, :, k], xg[:, :, k], s)
        return A.sqrt(s)
    pw = A.dt(f32(p))
    ip = A.div(one, pw)
    t = A.fn(np.power, np.abs(xg), pw)
    res = A.fn(np.power, seq(t), ip)
    over = np.isinf(t).any(axis=2) if A.dt is f32 else (np.abs(xg).astype(f32).astype(f64) ** f64(pw) > np.finfo(f32).max).any(axis=2)
    m = np.abs(xg).max(axis=2)
    with np.errstate(all="ignore"):
        inv = A.div(one, np.where(m > 0, m, one))
        t2 = A.fn(np.power, np.abs(A.mul(xg, inv[:, :, None])), pw)
        res2 = A.mul(A.fn(np.power, seq(t2), ip), m)
    return np.where(over, res2, res)


def group_deriv_model(A, x, y, g, p):
    yv = np.repeat(y, g, axis=1)
    if p == 1.0: return np.where(x == 0, A.dt(0), np.where(x > 0, A.dt(1), A.dt(-1)))
    pm, mp = A.sub(A.dt(f32(p)), A.dt(1)), A.sub(A.dt(1), A.dt(f32(p)))
    with np.errstate(all="ignore"):
        v = A.mul(A.mul(A.fn(np.power, np.abs(x), pm), A.fn(np.power, np.where(yv == 0, A.dt(1), yv), mp)), np.where(x >= 0, A.dt(1), A.dt(-1)))
    return np.where(yv == 0, A.dt(0), v)


def group_input(g, N=6, ngroups=7, huge=False):
    rng = rng_of("grp", g, huge)
    x = _draw(rng, (N, ngroups * g), "n")
    x[0, :g] = 0                      # an all-zero group
    if g > 1: x[1, g + 1] = 0         # a zero inside a non-zero group
    x[2, :] = -np.abs(x[2, :])
    if huge: x[3, :g] = f32(1e20) * (1 + np.arange(g, dtype=f32) / 8)
    return x


def group_pnorm_case(g, p):
    x = group_input(g, huge=(p == 3.0))
    ev = [group_pnorm_model(A, A.x(x) if A.name != "abs" else ARITH[0].x(x), g, p) for A in ARITH[:3]]
    if p == 0.0: exp, k = bits(ev[1]), "bits"
    elif p == 1.0: exp, k = bound(ev[0], g, ev[0]), g          # g additions of non-negative terms: S is the sum itself
    else: exp, k = ulp(ev[0], "pnorm"), ("ulp", "pnorm")
    cols = x.shape[1] // g
    ops = {"y": Operand(np.full((x.shape[0], cols), NAN, f32), cols + 3, 1, SENTINEL), "x": Operand(x, x.shape[1] + 2, 0, NAN)}
    case = Case("group_pnorm", "g%d-p%g" % (g, p), ops, dict(group=g, power=p), {"y": exp}, [{"y": e} for e in ev[1:]], "rescale" if p == 3.0 else "plain", k)
    if p > 0:
        xb = group_input(g)
        y32 = np.asarray(group_pnorm_model(ARITH[1], xb, g, p), f32)
        dv = [group_deriv_model(A, A.x(xb), A.x(y32), g, p) for A in ARITH[:3]]
        od = _draw(rng_of("grp-od", g, p), y32.shape, "n")
        case.deriv = dict(x=Operand(xb, xb.shape[1] + 2, 0, NAN), y=Operand(y32, y32.shape[1] + 5, 1, NAN), d=Operand(np.full(xb.shape, NAN, f32), xb.shape[1] + 2, 0, SENTINEL),
                          od=Operand(od, od.shape[1] + 4, 0, NAN), expect=bits(dv[1]) if p == 1.0 else ulp(dv[0], "pnorm_deriv"), evals=dv[1:])
        assert (y32[0, 0] == 0) and (dv[1][0, :g] == 0).all()
    return case


def group_max_case(g):
    rng = rng_of("gmax", g)
    x = rng.choice(np.array([-1.5, -0.25, 0.0, 0.5, 2.0], f32), (6, 7 * g)).astype(f32)      # ties
    y = np.maximum(x.reshape(6, 7, g).max(axis=2), f32(-1e20)).astype(f32)
    d = (x == np.repeat(y, g, axis=1)).astype(f32)
    od = _draw(rng, y.shape, "n")
    ops = {"y": Operand(np.full(y.shape, NAN, f32), 7 + 3, 1, SENTINEL), "x": Operand(x, 7 * g + 2, 0, NAN)}
    case = Case("group_max", "g%d" % g, ops, dict(group=g), {"y": bits(y)}, [{"y": y}], "max", "bits")
    case.deriv = dict(x=ops["x"], y=Operand(y, 7 + 5, 1, NAN), d=Operand(np.full(x.shape, NAN, f32), 7 * g + 2, 0, SENTINEL), od=Operand(od, 7 + 4, 0, NAN), expect=bits(d), evals=[d])
    return case


def elem_case(opname):
    """cudaF_max (in place), cudaF_equal_element_mask, cudaF_mul_rows_group_mat on pitched operands"""
    rng = rng_of(opname)
    vals = np.array([-1.5, -0.25, 0.0, 0.5, 2.0], f32)
    if opname == "max":
        a, b = rng.choice(vals, (9, 21)).astype(f32), rng.choice(vals, (9, 21)).astype(f32)
        out = np.where(b > a, b, a)
        return Case("max", "9x21", {"mat": Operand(a, 24, 1, SENTINEL), "A": Operand(b, 27, 0, NAN)}, {}, {"mat": bits(out)}, [{"mat": out}], "elem", "bits")
    if opname == "equal_element_mask":
        a, b = rng.choice(vals, (9, 21)).astype(f32), rng.choice(vals, (9, 21)).astype(f32)
        out = (a == b).astype(f32)
        return Case(opname, "9x21", {"m1": Operand(a, 24, 1, NAN), "m2": Operand(b, 27, 0, NAN), "mask": Operand(np.full(a.shape, NAN, f32), 22, 0, SENTINEL)}, {}, {"mask": bits(out)},
                    [{"mask": out}], "elem", "bits")
    y, x = _draw(rng, (6, 35), "n"), _draw(rng, (6, 7), "n")
    out = (y * np.repeat(x, 5, axis=1)).astype(f32)
    return Case("mul_rows_group_mat", "6x35-g5", {"y": Operand(y, 38, 1, SENTINEL), "x": Operand(x, 11, 0, NAN)}, dict(group=5), {"y": bits(out)}, [{"y": out}], "elem", "bits")


# ---- reduce_kernels.hip ------------------------------------------------------------------------------------------------------------------
OFFSET = f32(0.5)       # the mean offset of every summed input: a dropped or doubled term is then far outside the bound


def _sum_bound(terms64, alpha, beta, v, n_roundings):
    """alpha * sum + beta v; S = |alpha| sum |x| + |beta v|"""
    a, b = f64(f32(alpha)), f64(f32(beta))
    ref = a * terms64.sum(axis=-1) + (b * v.astype(f64) if beta != 0 else 0.0)
    S = abs(a) * np.abs(terms64).sum(axis=-1) + (np.abs(b * v.astype(f64)) if beta != 0 else 0.0)
    return bound(ref, n_roundings, S)


def _sum32(terms, alpha, beta, v, fold):
    """a plain float32 evaluation: ascending sum, then the epilogue"""
    acc = np.zeros(terms.shape[:-1], f32)
    for j in range(terms.shape[-1]):
        acc = (acc + terms[..., j]).astype(f32)
    A = ARITH[2] if fold else ARITH[1]
    if beta == 0: return A.mul(f32(alpha), acc)
    return A.muladd(f32(alpha), acc, A.mul(f32(beta), v))


def col_sum_case(rows, cols, beta):
    """aslp_add_col_sum_mat_vec: v[r] = alpha sum_c M[r][c] + beta v[r]; k = cols + 3 (the sum, alpha ., beta ., +)"""
    rng = rng_of("colsum", rows, cols, beta)
    M, v0, alpha = (_draw(rng, (rows, cols), "n") + OFFSET).astype(f32), _draw(rng, (rows,), "n"), -0.75
    vin = v0 if beta != 0 else np.full(rows, NAN, f32)
    exp = _sum_bound(M.astype(f64), alpha, beta, v0, cols + 3)
    return Case("add_col_sum_mat_vec", "%dx%d-b%g" % (rows, cols, beta), {"M": Operand(M, cols + 3, 1, NAN), "v": Operand(vin, None, 1, SENTINEL)}, dict(alpha=alpha, beta=beta),
                {"v": exp}, [{"v": _sum32(M, alpha, beta, v0, f)} for f in (0, 1)], "gs" if rows > 2048 * 4 else "one", cols + 3)


def row_sum_vec_case(rows, cols, beta, sgd):
    """aslp_add_row_sum_mat_vec(_sgd): v[c] = alpha sum_r M[r][c] + beta v[c]; w[c] += w_alpha v[c].  k = rows + 3 for v, + 2 for w"""
    rng = rng_of("rowsumvec", rows, cols, beta, sgd)
    M, v0, w0, alpha, wa = (_draw(rng, (rows, cols), "n") + OFFSET).astype(f32), _draw(rng, (cols,), "n"), _draw(rng, (cols,), "n"), 0.5, -0.125
    vin = v0 if beta != 0 else np.full(cols, NAN, f32)
    ev = _sum_bound(M.T.astype(f64), alpha, beta, v0, rows + 3)
    ops = {"M": Operand(M, cols + (4 if cols % 4 == 0 else 3), 0, NAN), "v": Operand(vin, None, 1, SENTINEL)}
    v32 = [_sum32(M.T, alpha, beta, v0, f) for f in (0, 1)]
    expect, evals = {"v": ev}, [{"v": a} for a in v32]
    if sgd:
        ops["w"] = Operand(w0, None, 0, SENTINEL)
        expect["w"] = bound(w0.astype(f64) + f64(f32(wa)) * ev[1], rows + 5, np.abs(w0.astype(f64)) + abs(f64(f32(wa))) * ev[3])
        for e, A in zip(evals, ARITH[1:3]): e["w"] = A.muladd(f32(wa), e["v"], w0)
    vec = ops["M"].addr() % 16 == 0 and ops["M"].ld % 4 == 0 and cols % 4 == 0
    return Case("add_row_sum_mat_vec" + ("_sgd" if sgd else ""), "%dx%d-b%g" % (rows, cols, beta), ops, dict(alpha=alpha, beta=beta, w_alpha=wa), expect, evals, path_name(vec, 0), rows + 3)


def matrix_sum_case(rows, cols=37):
    M = (_draw(rng_of("msum", rows), (rows, cols), "n") + OFFSET).astype(f32)
    ref, S = M.astype(f64).sum(), np.abs(M.astype(f64)).sum()
    return Case("matrix_sum", "%dx%d" % (rows, cols), {"M": Operand(M, cols + 3, 1, NAN), "out": Operand(np.full(1, np.nan, f64), None, 0, f64(SENTINEL))}, {},
                {"out": bound(ref, max(rows * cols, 1), S, 2.0 ** -53)}, [{"out": np.array([ref])}], "gs" if rows > 2048 * 4 else "one", "n, in double")


def vec_sum_case(dim, inc):
    x = (_draw(rng_of("vsum", dim, inc), (dim, 1), "n") + OFFSET).astype(f32)
    ref, S = x.astype(f64).sum(), np.abs(x.astype(f64)).sum()
    return Case("vec_sum", "n%d-inc%d" % (dim, inc), {"v": Operand(x, inc, 1, NAN), "value": Operand(np.full(1, NAN, f32), None, 1, SENTINEL)}, dict(dim=dim, inc=inc),
                {"value": bound(ref, max(dim, 1), S)}, [{"value": _sum32(x[:, 0][None, :], 1.0, 0.0, None, f)} for f in (0, 1)], "one", "n")


def diag_mat_mat_case(trans, n, v_dim, beta=0.5):
    """v[i] = alpha sum_j M'[i][j] N'[j][i] + beta v[i]; trans 1: M is stored [n x v_dim] and read transposed, trans 2: N is stored [v_dim x n] and
    read transposed.  k = 2 n + 3"""
    rng = rng_of("diagmm", trans, n, v_dim, beta)
    Mm, Nm = (_draw(rng, (v_dim, n), "n") + OFFSET).astype(f32), (_draw(rng, (n, v_dim), "n") + OFFSET).astype(f32)
    v0, alpha = _draw(rng, (v_dim,), "n"), 0.75
    terms = Mm.astype(f64) * Nm.T.astype(f64)
    exp = _sum_bound(terms, alpha, beta, v0, 2 * n + 3)
    evals = []
    for fold in (0, 1):
        A, acc = ARITH[2] if fold else ARITH[1], np.zeros(v_dim, f32)
        for j in range(n): acc = A.muladd(Mm[:, j], Nm[j, :], acc)
        evals.append({"v": A.mul(f32(alpha), acc) if beta == 0 else A.muladd(f32(alpha), acc, A.mul(f32(beta), v0))})
    Ms, Ns = Mm.T.copy() if trans == 1 else Mm, Nm.T.copy() if trans == 2 else Nm
    ops = {"v": Operand(v0 if beta != 0 else np.full(v_dim, NAN, f32), None, 1, SENTINEL), "M": Operand(Ms, Ms.shape[1] + 3, 0, NAN), "N": Operand(Ns, Ns.shape[1] + 2, 1, NAN)}
    return Case("add_diag_mat_mat", "%s-n%d-v%d-b%g" % ("NTt"[trans], n, v_dim, beta), ops, dict(alpha=alpha, beta=beta, trans=trans, n=n), {"v": exp}, evals, "diag", 2 * n + 3)


def row_sum_mat_case(P, cols, pitch, off, beta):
    """cudaF_add_row_sum_mat: dst[j][c] = alpha sum_{k<P} src[j P + k][c] + beta dst[j][c]; k = P + 3"""
    rng = rng_of("rowsummat", P, cols, pitch, off, beta)
    rows = 5
    src, d0, alpha = (_draw(rng, (rows * P, cols), "n") + OFFSET).astype(f32), _draw(rng, (rows, cols), "n"), -0.75
    terms = src.reshape(rows, P, cols).transpose(0, 2, 1)
    exp = _sum_bound(terms.astype(f64), alpha, beta, d0, P + 3)
    ops = {"dst": Operand(d0 if beta != 0 else np.full((rows, cols), NAN, f32), pitch, off, SENTINEL), "src": Operand(src, pitch + (4 if pitch % 4 == 0 else 3), 0, NAN)}
    vec = vec_path(cols, [(o.addr(), o.ld) for o in ops.values()])
    return Case("add_row_sum_mat", "P%d-%dx%d-ld%d-off%d-b%g" % (P, rows, cols, pitch, off, beta), ops, dict(P=P, alpha=alpha, beta=beta), {"dst": exp},
                [{"dst": _sum32(terms, alpha, beta, d0, f)} for f in (0, 1)], path_name(vec, 0), P + 3)


def conv_mme_case(C, beta):
    """cudaF_add_conv_mat_mat_elements: dst[k C + c] = alpha A[k + c] .* B[c] + beta dst; k = 4 (beta == 0: 2)"""
    rng = rng_of("convmme", C, beta)
    K, cols, alpha = 6, 23, 0.7
    A_, B_, d0 = _draw(rng, (K + C - 1, cols), "n"), _draw(rng, (C, cols), "n"), _draw(rng, (K * C, cols), "n")
    ai = (np.arange(K * C) // C) + (np.arange(K * C) % C)
    a, b = A_[ai], B_[np.arange(K * C) % C]
    if beta == 0:
        exp, ev = evaluate(lambda A, a, b: A.mul(A.mul(A.c(alpha), a), b), (a, b), 2)
    else:
        exp, ev = evaluate(lambda A, d, a, b: A.muladd(A.mul(A.c(alpha), a), b, A.mul(A.c(beta), d)), (d0, a, b), 4)
    ops = {"dst": Operand(d0 if beta != 0 else np.full(d0.shape, NAN, f32), cols + 3, 1, SENTINEL), "A": Operand(A_, cols + 5, 0, NAN), "B": Operand(B_, cols + 1, 0, NAN)}
    return Case("add_conv_mat_mat_elements", "C%d-b%g" % (C, beta), ops, dict(C=C, alpha=alpha, beta=beta), {"dst": exp}, [{"dst": e} for e in ev], "conv", 4 if beta else 2)


MAX_NORM = 2.0


def max_norm_input(rows, cols):
    """rows below, at and above the norm and a zero row"""
    x = _draw(rng_of("maxnorm", rows, cols), (rows, cols), "n")
    n = np.sqrt((x.astype(f64) ** 2).sum(axis=1))
    target = np.where(np.arange(rows) % 3 == 0, 0.5 * MAX_NORM, np.where(np.arange(rows) % 3 == 1, 3.0 * MAX_NORM, MAX_NORM))
    x = (x * (target / np.where(n > 0, n, 1))[:, None]).astype(f32)
    if rows > 3: x[3] = 0
    return x


def max_norm_check(before, after, max_norm=MAX_NORM):
    """afterwards every row's float64 norm is <= max_norm (1 + 4 u); rows whose norm was clearly below are bit-identical; a scaled row is its input
    times one factor (the direction is kept to float32 rounding)"""
    fails = []
    nb, na = (np.sqrt((a.astype(f64) ** 2).sum(axis=1)) for a in (before, after))
    if not (na <= max_norm * (1 + 4 * U)).all():
        fails.append("row %d has norm %.9g > %g (1 + 4u)" % (int(na.argmax()), na.max(), max_norm))
    below = nb < max_norm * (1 - 1e-5)
    if not np.array_equal(_bits(after[below]), _bits(before[below])):
        fails.append("a row below the norm was changed")
    above = nb > max_norm * (1 + 1e-5)
    if above.any():
        want = before[above].astype(f64) * (max_norm / nb[above])[:, None]
        if not (np.abs(after[above] - want) <= 8 * U * np.abs(want) + 1e-30).all():
            fails.append("a scaled row is not its input times max_norm / norm")
        if not (na[above] >= max_norm * (1 - 16 * U)).all():
            fails.append("a scaled row ends below the norm")
    at = ~below & ~above        # a row at the norm: its input times one factor in [1 - 8u, 1] (the computed norm is within a few u of max_norm), each product rounded once
    a, b = np.abs(after[at].astype(f64)), np.abs(before[at].astype(f64))
    if not ((a <= b) & (a >= b * (1 - 9 * U)) & (np.signbit(after[at]) == np.signbit(before[at]))).all():
        fails.append("a row at the norm is not its input times one factor in [1 - 8u, 1]")
    return fails


def max_norm_judge(op, got_image, before, max_norm=MAX_NORM):
    """max_norm_check on the view of a buffer as it came back, and every word outside the view as it was"""
    fails = max_norm_check(before, op.view(got_image).copy(), max_norm)
    keep = np.array(got_image)
    op.view(keep)[...] = before
    if not np.array_equal(_bits(keep), _bits(op.image)):
        fails.append("words outside the view changed")
    return fails


def max_norm_f32(x, max_norm=MAX_NORM):
    s = np.zeros(x.shape[0], f32)
    for c in range(x.shape[1]): s = (s + (x[:, c] * x[:, c]).astype(f32)).astype(f32)
    scl = (np.sqrt(s).astype(f32) * (f32(1) / f32(max_norm))).astype(f32)
    scl = (f32(1) / np.maximum(scl, f32(1))).astype(f32)
    return (x * scl[:, None]).astype(f32)


# ---- optim_kernels.hip -------------------------------------------------------------------------------------------------------------------
SOLVERS = ["sgd", "momentum", "adagrad", "rmsprop", "adadelta", "adam"]
SOD_PAR = dict(lr=0.01, momentum=0.9, gamma=0.95, beta1=0.9, beta2=0.999, corr1=1.25, corr2=1.5)
SOD_N = [1, 257, 524325]


def sod_step(solver, g, p, s1, s2, par=SOD_PAR):
    """one step in float64 in the order of aslp-parallel/optimizer.h as csrc/optim_kernels.hip cites it, from float32 state -> {name: (ref, k, S)}.
    k counts the fp32 roundings on the way to each output (a square root or division counts one; an error in G enters 1 / sqrt(G) halved)"""
    c = {k: f64(f32(v)) for k, v in par.items()}
    g, p, s1, s2 = (a.astype(f64) for a in (g, p, s1, s2))
    fl = lambda v: np.maximum(v, f64(f32(1e-8)))
    out = {}
    if solver == "sgd":
        step = c["lr"] * g; k = 2
    elif solver == "momentum":
        m = c["lr"] * g + c["momentum"] * s1
        out["s1"] = (m, 3, np.abs(c["lr"] * g) + np.abs(c["momentum"] * s1))
        out["param"] = (p - m, 4, np.abs(p) + out["s1"][2])      # the two products may cancel in m: their magnitudes, not |m|, carry its error
        return out
    elif solver in ("adagrad", "rmsprop"):
        a, b = (1.0, 1.0) if solver == "adagrad" else (f64(f32(0.1)), f64(f32(0.9)))
        G = a * g * g + b * s1
        out["s1"] = (G, 4, G)
        step = c["lr"] * (g / np.sqrt(fl(G))); k = 4 + 5
    elif solver == "adadelta":
        om = f64(f32(1) - f32(par["gamma"]))
        G = om * g * g + c["gamma"] * s1
        out["s1"] = (G, 4, G)
        step = (1.0 / np.sqrt(fl(G))) * np.sqrt(fl(s2)) * g; k = 4 + 6
        D = om * step * step + c["gamma"] * s2
        out["s2"] = (D, 2 * 9 + 4, D)
    else:
        o1, o2 = f64(f32(1) - f32(par["beta1"])), f64(f32(1) - f32(par["beta2"]))
        m = o1 * g + c["beta1"] * s1
        v = o2 * g * g + c["beta2"] * s2
        out["s1"], out["s2"] = (m, 3, np.abs(o1 * g) + np.abs(c["beta1"] * s1)), (v, 4, v)
        lrc = f64(f32(par["lr"]) * f32(par["corr1"]))
        den = np.sqrt(fl(v * c["corr2"]))
        step = lrc * (np.abs(o1 * g) + np.abs(c["beta1"] * s1)) / den      # magnitude: m may cancel
        out["param"] = (p - lrc * (m / den), 4 + 8, np.abs(p) + step)
        return out
    out["param"] = (p - step, k, np.abs(p) + np.abs(step))
    return out


def sod_inputs(solver, n):
    rng = rng_of("sod", solver, n)
    g = [_draw(rng, (n,), "n") for _ in range(2)]
    for a in g:
        a[np.abs(a) < 1e-2] = f32(0.25)
        a[::5] = 0                       # zero gradients: G stays 0 and the 1e-8 floor is what the square root sees
    p = _draw(rng, (n,), "n")
    return g, p, np.zeros(n, f32), np.zeros(n, f32)


# ---- every case ---------------------------------------------------------------------------------------------------------------------------
def table():
    """[(id, builder)] of every table case (the optimiser steps and max_norm_rows have their own drivers); built on demand"""
    t = map_table() + row_gather_table()
    one = lambda f, *a: t.append(("%s%s" % (f.__name__[:-5], "".join("-%s" % (x,) for x in a)), (lambda f=f, a=a: f(*a))))
    one(add_mat_trans_case), one(add_mat_diag_vec_strided_case), one(regularize_l1_case), one(set_const_i32_case), one(scatter_add_case)
    for o in ("copy_cols", "add_cols", "copy"): one(col_gather_case, o)
    for s in SPLICE:
        one(splice_case, 0, *s), one(splice_case, 1, *s)
    for n in VEC_N:
        one(f2d_case, n), one(d2f_case, n)
        for o in ("add_vec_vec", "vec_axpy", "vec_axpy2", "vec_diff"): one(vec_case, o, n)
    for d in DROPOUT: one(dropout_case, *d)
    for g in CONV:
        one(conv_case, 0, *g), one(conv_case, 1, *g)
    one(conv_case, 0, *CONV_GS_GATHER), one(conv_case, 1, *CONV_GS_INDIFF)
    for g in POOL: one(maxpool_case, *g)
    for nd in LN_CASES: one(length_norm_case, *nd)
    for g in GROUPS:
        for p in POWERS: one(group_pnorm_case, g, p)
        one(group_max_case, g)
    for o in ("max", "equal_element_mask", "mul_rows_group_mat"): one(elem_case, o)
    for cols in (1, 63, 64, 65, 1000):
        for rows in (1, 4, 5, 8200):       # 8200 rows: past 2048 blocks x 4 waves; at 1000 columns a 33 MB operand, the largest of the file
            for beta in (0.0, 0.5): one(col_sum_case, rows, cols, beta)
    for rows in (0, 1, 5, 8200): one(matrix_sum_case, rows)
    for dim in (0, 1, 255, 256, 257, 5000):
        for inc in (1, 3): one(vec_sum_case, dim, inc)
    for trans in (0, 1, 2):
        for n in (1, 16, 17, 100):
            for v in (1, 64, 65): one(diag_mat_mat_case, trans, n, v, 0.5 if (n + v) % 2 else 0.0)
    for P in (1, 4, 7):
        for cols, pitch, off in ((64, 72, 0), (64, 72, 1), (53, 53, 0)):
            for beta in (0.0, 0.5): one(row_sum_mat_case, P, cols, pitch, off, beta)
    for C in (1, 7):
        for beta in (0.0, 0.3): one(conv_mme_case, C, beta)
    for rows, cols in ((1, 1), (37, 53), (40, 64), (600, 128)):
        for beta in (0.0, 0.5): one(row_sum_vec_case, rows, cols, beta, 1)
    one(row_sum_vec_case, 37, 64, 0.0, 0), one(row_sum_vec_case, 37, 53, 0.5, 0)
    assert len(set(i for i, _ in t)) == len(t)
    return t


MAX_NORM_SHAPES = [(7, 1), (7, 64), (7, 65), (7, 300), (8200, 64)]
