"""GPU parity: every substrate kernel of libaslp_hip.so (called through the C ABI) against the
CPU oracle on the same seeded inputs.  Mirrors the reference's CPU-vs-device differential
tests (aslp-cudamatrix/cu-matrix-test.cc:2605-2636, cu-math-test.cc).  Tolerances: bit-exact
for index/copy ops; 1e-4 relative (BASELINE.json north_star) for fp32 math -- most ops are
far tighter and assert 1e-5/1e-6."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-4  # north_star: fp32 within 1e-4 relative


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def strided(rows, cols, stride, dev, fill=None):
    """A [rows x cols] view into a wider buffer, like the reference's pitched CuMatrix."""
    buf = torch.full((rows, stride), float("nan"), device=dev)
    v = buf[:, :cols]
    if fill is not None:
        v.copy_(T(fill, dev))
    return v


@pytest.mark.parametrize("rows,cols,stride", [(100, 111, 111), (100, 112, 128), (1, 1, 1), (257, 2048, 2048)])
def test_sigmoid_tanh_and_diffs(aslp, oracle, dev, rows, cols, stride):
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((rows, cols)) * 4).astype(np.float32)
    e = rng.standard_normal((rows, cols)).astype(np.float32)
    xd = strided(rows, cols, stride, dev, x)
    for name, dname in (("sigmoid", "diff_sigmoid"), ("tanh", "diff_tanh")):
        y = strided(rows, cols, stride, dev)
        getattr(aslp.ops, name)(y, xd)
        ref = oracle.unary("orc_" + name, x)
        assert oracle.rel_err(y.cpu().numpy(), ref) < 1e-6
        # the reference's UnitTestCuSigmoid closed form (cu-matrix-test.cc:1925-1948)
        if name == "sigmoid":
            assert oracle.rel_err(y.cpu().numpy(), 1.0 / (1.0 + np.exp(-x.astype(np.float64)))) < 1e-6
        eo = strided(rows, cols, stride, dev)
        getattr(aslp.ops, dname)(eo, y, T(e, dev))
        dref = oracle.binary("orc_" + dname, y.cpu().numpy(), e)
        assert oracle.rel_err(eo.cpu().numpy(), dref) < 1e-6


def test_sigmoid_extremes_no_nan(aslp, dev):
    x = torch.tensor([[-1e4, -100.0, -88.0, 0.0, 88.0, 100.0, 1e4, float("inf")]], device=dev)
    y = torch.empty_like(x)
    aslp.ops.sigmoid(y, x)
    assert torch.isfinite(y).all() and y[0, 0] == 0 and y[0, -2] == 1
    aslp.ops.tanh(y, x)
    assert torch.isfinite(y).all() and y[0, 0] == -1 and y[0, -2] == 1


@pytest.mark.parametrize("rows,cols", [(37, 10), (49, 59), (64, 128), (33, 513), (1024, 3000), (3, 9000)])
def test_softmax(aslp, oracle, dev, rows, cols):
    rng = np.random.default_rng(2)
    x = (rng.standard_normal((rows, cols)) * 5).astype(np.float32)  # UnitTestCuSoftmax scales by 5
    y = torch.empty(rows, cols, device=dev)
    aslp.ops.softmax(y, T(x, dev))
    ref = oracle.unary("orc_softmax_rows", x)
    assert oracle.rel_err(y.cpu().numpy(), ref) < 1e-5  # the reference's own bar (cu-matrix-test.cc:2009)
    assert np.allclose(y.sum(1).cpu().numpy(), 1.0, atol=1e-5)


@pytest.mark.parametrize("rows,in_cols,offs", [(7, 5, [-2, 0, 3]), (300, 40, list(range(-5, 6))), (1, 8, [-1, 1]),
                                                 (129, 24, [0]), (200, 13, [-199, 250, 0, 0])])
def test_splice_bit_exact(aslp, oracle, dev, rows, in_cols, offs):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((rows, in_cols)).astype(np.float32)
    off = np.asarray(offs, np.int32)
    y = torch.empty(rows, in_cols * len(offs), device=dev)
    aslp.ops.splice(y, T(x, dev), T(off, dev))
    assert np.array_equal(y.cpu().numpy(), oracle.splice(x, off))  # bit-exact
    # reference unit test's expectation (cu-math-test.cc:123-138): clamped row copy
    for k, o in enumerate(offs):
        src = np.clip(np.arange(rows) + o, 0, rows - 1)
        assert np.array_equal(y.cpu().numpy()[:, k * in_cols:(k + 1) * in_cols], x[src])
    od = rng.standard_normal((rows, in_cols * len(offs))).astype(np.float32)
    idf = torch.empty(rows, in_cols, device=dev)
    aslp.ops.splice_backward(idf, T(od, dev), T(off, dev))
    ref = oracle.splice_backprop(od, in_cols, off)
    assert oracle.rel_err(idf.cpu().numpy(), ref) < 1e-6


def test_randomize_bit_exact(aslp, oracle, dev):
    rng = np.random.default_rng(4)
    x = rng.standard_normal((500, 440)).astype(np.float32)
    idx = rng.permutation(500).astype(np.int32)[:300]
    y = torch.zeros(500, 440, device=dev)
    aslp.ops.randomize(y, T(x, dev), T(idx, dev))
    assert np.array_equal(y.cpu().numpy()[:300], x[idx])
    assert (y[300:] == 0).all()


@pytest.mark.parametrize("rows,cols", [(150, 233), (4, 3), (1024, 3000), (5, 600)])
def test_find_row_max_id(aslp, oracle, dev, rows, cols):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((rows, cols)).astype(np.float32)
    x[0, :] = 0.5  # all ties: first index wins (cu-matrix.cc:1500-1505 strict '<')
    if cols > 300:
        x[1, 7] = x[1, 299] = 9.0
    ids = aslp.ops.find_row_max_id(T(x, dev)).cpu().numpy()
    assert np.array_equal(ids, oracle.find_row_max_id(x))
    assert ids[0] == 0
    # running per-256-column form with the reference's call pattern (cu-matrix.cc:1480-1499)
    xd = T(x, dev)
    val = torch.full((rows,), -1e21, device=dev)
    idt = torch.full((rows,), -1, dtype=torch.int32, device=dev)
    d = aslp.ops.dim(xd)
    for blk in range(cols // 256):
        aslp.lib.cudaF_find_row_max_id(aslp.Dim3(1, rows, 1), aslp.Dim3(256, 1, 1), C.c_void_p(xd.data_ptr() + 4 * 256 * blk),
                                       aslp.ops.ptr(val), aslp.ops.ptr(idt), 256 * blk, d)
    if cols % 256:
        off = (cols // 256) * 256
        aslp.lib.cudaF_find_row_max_id(aslp.Dim3(1, rows, 1), aslp.Dim3(cols % 256, 1, 1), C.c_void_p(xd.data_ptr() + 4 * off),
                                       aslp.ops.ptr(val), aslp.ops.ptr(idt), off, d)
    aslp.check_error()
    assert np.array_equal(idt.cpu().numpy(), ids)


GEMM_SHAPES = [
    # (M, N, K)
    (37, 41, 29), (1, 1, 1), (128, 128, 16), (130, 70, 33), (256, 2048, 440), (64, 3000, 512),
    (32, 2048, 256), (8, 64, 40), (200, 96, 1000), (1024, 512, 2048),
    (256, 512, 1920), (100, 72, 1100), (1920, 256, 2048),  # long K on a small grid: split-K + ordered reduce
]


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
@pytest.mark.parametrize("tA,tB", [(0, 1), (0, 0), (1, 0), (1, 1)])
def test_sgemm_vs_oracle(aslp, oracle, dev, M, N, K, tA, tB):
    rng = np.random.default_rng(M * 7 + N * 3 + K + tA * 2 + tB)
    A = rng.standard_normal((K, M) if tA else (M, K)).astype(np.float32)
    B = rng.standard_normal((N, K) if tB else (K, N)).astype(np.float32)
    C0 = rng.standard_normal((M, N)).astype(np.float32)
    for alpha, beta in ((1.0, 0.0), (0.7, 1.3)):
        Cd = T(C0, dev)
        if beta == 0.0:
            Cd.fill_(float("nan"))  # beta == 0 must not read C
        aslp.ops.sgemm(tA, tB, alpha, T(A, dev), T(B, dev), beta, Cd)
        ref = oracle.add_mat_mat(C0, alpha, A, tA, B, tB, beta)
        assert oracle.rel_err(Cd.cpu().numpy(), ref) < 2e-6, (M, N, K, tA, tB, alpha, beta)


def test_sgemm_asymmetric_identity(aslp, dev):
    """A = I with an asymmetric B catches a transposed C write (cdna guide G9)."""
    n = 96
    B = torch.arange(n * n, dtype=torch.float32, device=dev).reshape(n, n) / 100.0
    I = torch.eye(n, device=dev)
    Cm = torch.empty(n, n, device=dev)
    aslp.ops.sgemm(0, 0, 1.0, I, B, 0.0, Cm)
    assert torch.equal(Cm, B)
    aslp.ops.sgemm(0, 1, 1.0, I, B, 0.0, Cm)
    assert torch.equal(Cm, B.t())
    aslp.ops.sgemm(1, 0, 1.0, B, I, 0.0, Cm)
    assert torch.equal(Cm, B.t())


def test_sgemm_strided_views_unaligned(aslp, oracle, dev):
    """Sub-matrix views (ColRange/RowRange of LSTM buffers): odd column offsets force the scalar path."""
    rng = np.random.default_rng(11)
    big = rng.standard_normal((70, 131)).astype(np.float32)
    W = rng.standard_normal((50, 37)).astype(np.float32)
    bd = T(big, dev)
    A = bd[3:3 + 60, 5:5 + 37]  # unaligned pointer, stride 131
    out = torch.zeros(64, 77, device=dev)
    Cv = out[2:62, 9:59]
    aslp.ops.sgemm(0, 1, 1.0, A, T(W, dev), 0.0, Cv)
    ref = big[3:63, 5:42] @ W.T
    assert oracle.rel_err(Cv.cpu().numpy(), ref) < 2e-6
    mask = torch.ones_like(out, dtype=torch.bool)
    mask[2:62, 9:59] = False
    assert (out[mask] == 0).all()  # nothing outside the view was touched


def test_sgemm_epilogue(aslp, oracle, dev):
    rng = np.random.default_rng(12)
    M, N, K = 100, 72, 64
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = rng.standard_normal((N, K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    out = torch.empty(M, N, device=dev)
    act = torch.empty(M, N, device=dev)
    bd = T(b, dev)
    ep = aslp._lib.GemmEpilogue(bd.data_ptr(), 0.0, None, 0, 0.0, act.data_ptr(), N, 1)
    aslp.ops.sgemm(0, 1, 1.0, T(A, dev), T(W, dev), 0.0, out, ep)
    ref = A @ W.T + b
    assert oracle.rel_err(out.cpu().numpy(), ref) < 2e-6
    assert oracle.rel_err(act.cpu().numpy(), oracle.unary("orc_sigmoid", out.cpu().numpy())) < 1e-6
    # SGD epilogue: G = diff^T in + mmt*G, clipped; W += -lr*G
    diff = rng.standard_normal((M, N)).astype(np.float32)
    G0 = rng.standard_normal((N, K)).astype(np.float32)
    Gd, Wd = T(G0, dev), T(W, dev)
    ep = aslp._lib.GemmEpilogue(None, 5.0, Wd.data_ptr(), K, -0.01, None, 0, 0)
    aslp.ops.sgemm(1, 0, 1.0, T(diff, dev), T(A, dev), 0.9, Gd, ep)
    Gref = np.clip(diff.T @ A + 0.9 * G0, -5, 5)
    assert oracle.rel_err(Gd.cpu().numpy(), Gref) < 2e-6
    assert oracle.rel_err(Wd.cpu().numpy(), W - 0.01 * Gref) < 2e-6
    # the same epilogue behind a split-K product (recurrent weight gradient: 1920 frames, 256 x 512 output), run twice:
    # the chunk-ordered reduction makes it reproducible to the bit
    M, N, K = 1920, 256, 512
    diff = rng.standard_normal((M, N)).astype(np.float32)
    A = rng.standard_normal((M, K)).astype(np.float32)
    G0 = rng.standard_normal((N, K)).astype(np.float32)
    W = rng.standard_normal((N, K)).astype(np.float32)
    res = []
    for _ in range(2):
        Gd, Wd = T(G0, dev), T(W, dev)
        ep = aslp._lib.GemmEpilogue(None, 40.0, Wd.data_ptr(), K, -0.01, None, 0, 0)
        aslp.ops.sgemm(1, 0, 1.0, T(diff, dev), T(A, dev), 0.9, Gd, ep)
        res.append((Gd.cpu().numpy(), Wd.cpu().numpy()))
    Gref = np.clip(diff.astype(np.float64).T @ A + 0.9 * G0, -40, 40)
    assert (np.abs(Gref) == 40).any() and (np.abs(Gref) < 40).any()
    assert oracle.rel_err(res[0][0], Gref) < 2e-6
    assert oracle.rel_err(res[0][1], W - 0.01 * Gref) < 2e-6
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


@pytest.mark.parametrize("mb,n_out,n_in", [(100, 72, 64), (1024, 2048, 440), (256, 3000, 128), (60, 130, 36), (33, 40, 20)])
def test_sgemm_colsum_epilogue(aslp, oracle, dev, mb, n_out, n_in):
    """Bias gradient + bias SGD step folded into the weight-gradient GEMM (AffineTransform::Update,
    nnet-affine-transform.h:214-227): colsum = sum_k diff[k][:] + mmt*colsum ; bias += -lr*colsum."""
    rng = np.random.default_rng(mb + n_out)
    diff = rng.standard_normal((mb, n_out)).astype(np.float32)
    x = rng.standard_normal((mb, n_in)).astype(np.float32)
    G0 = rng.standard_normal((n_out, n_in)).astype(np.float32)
    bc0 = rng.standard_normal(n_out).astype(np.float32)
    b0 = rng.standard_normal(n_out).astype(np.float32)
    Gd, bcd, bd = T(G0, dev), T(bc0, dev), T(b0, dev)
    ep = aslp._lib.GemmEpilogue(None, 0.0, None, 0, 0.0, None, 0, 0, bcd.data_ptr(), 0.9, bd.data_ptr(), -0.02)
    aslp.ops.sgemm(1, 0, 1.0, T(diff, dev), T(x, dev), 0.5, Gd, ep)
    assert oracle.rel_err(Gd.cpu().numpy(), diff.T.astype(np.float64) @ x + 0.5 * G0) < 2e-6
    bc_ref = diff.astype(np.float64).sum(0) + 0.9 * bc0
    assert oracle.rel_err(bcd.cpu().numpy(), bc_ref) < 2e-6
    assert oracle.rel_err(bd.cpu().numpy(), b0 - 0.02 * bc_ref) < 2e-6
    # column sums of a non-transposed A are not defined
    with pytest.raises(ValueError):
        aslp.ops.sgemm(0, 0, 1.0, T(x, dev), T(rng.standard_normal((n_in, 8)).astype(np.float32), dev), 0.0, torch.empty(mb, 8, device=dev), ep)


# On 256 CUs: (64, 32) (5, 16) run the panel-resident kernels at 4 row slots and (300, 48) at 8; (1024, 2048) runs the cooperative kernels
# (Q = 4 workgroups per panel, 8 slots); (8, 6) (100, 37) (129, 260) (1025, 64) the three-launch path.  bn_*_panel<4, 16> and the other
# cooperative shapes: tests/test_bn_xent_kernels_gpu.py.
@pytest.mark.parametrize("rows,cols", [(8, 6), (64, 32), (1024, 2048), (100, 37), (129, 260), (300, 48), (1025, 64), (5, 16)])
def test_batchnorm_forward_backward(aslp, oracle, dev, rows, cols):
    rng = np.random.default_rng(6)
    x = (rng.standard_normal((rows, cols)) * 2 + 0.5).astype(np.float32)
    dy = rng.standard_normal((rows, cols)).astype(np.float32)
    bn = oracle.Bn(cols)
    bn.scale[:] = rng.uniform(0.5, 1.5, cols)
    bn.shift[:] = rng.standard_normal(cols)
    bn.dscale[:] = rng.standard_normal(cols)
    bn.dshift[:] = rng.standard_normal(cols)
    dsc0, dsh0 = bn.dscale.copy(), bn.dshift.copy()
    ref_out = bn.propagate(x)
    ref_xhat = bn.xs.copy()
    xd = T(x, dev)
    out, xhat = torch.empty_like(xd), torch.empty_like(xd)
    scale, shift = T(bn.scale, dev), T(bn.shift, dev)
    mean, inv = torch.empty(cols, device=dev), torch.empty(cols, device=dev)
    accm = torch.zeros(cols, dtype=torch.float64, device=dev)
    accv = torch.zeros(cols, dtype=torch.float64, device=dev)
    aslp.ops.bn_forward(xd, out, xhat, scale, shift, mean, inv, accm, accv)
    assert oracle.rel_err(out.cpu().numpy(), ref_out) < 1e-5
    assert oracle.rel_err(xhat.cpu().numpy(), ref_xhat) < 1e-5
    assert oracle.rel_err(mean.cpu().numpy(), bn.mean) < 1e-5
    assert oracle.rel_err(inv.cpu().numpy(), bn.var) < 1e-5
    assert oracle.rel_err(accm.cpu().numpy(), bn.acc_means) < 1e-12 * rows + 1e-9
    assert oracle.rel_err(accv.cpu().numpy(), bn.acc_vars) < 1e-12 * rows + 1e-9
    ref_idf = bn.backpropagate(x, dy, 0.9)
    dsc, dsh = T(dsc0, dev), T(dsh0, dev)
    idf = torch.empty_like(xd)
    aslp.ops.bn_backward(xd, T(dy, dev), xhat, scale, mean, inv, dsc, dsh, 0.9, idf)
    assert oracle.rel_err(idf.cpu().numpy(), ref_idf) < TOL
    assert oracle.rel_err(dsc.cpu().numpy(), bn.dscale) < 1e-5
    assert oracle.rel_err(dsh.cpu().numpy(), bn.dshift) < 1e-5


# (5, 8192): the widest row the register-cached kernels hold; (6, 8193) and (4, 20000): the streaming kernel beyond (the reference has no limit)
@pytest.mark.parametrize("rows,cols", [(16, 10), (256, 3000), (100, 128), (5, 8192), (6, 8193), (4, 20000)])
def test_xent_eval(aslp, oracle, dev, rows, cols):
    rng = np.random.default_rng(7)
    logits = rng.standard_normal((rows, cols)).astype(np.float32) * 3
    y = oracle.unary("orc_softmax_rows", logits)
    labels = rng.integers(0, cols, rows).astype(np.int32)
    tgt = np.zeros((rows, cols), np.float32)
    tgt[np.arange(rows), labels] = 1.0
    fw = rng.uniform(0.0, 1.0, rows).astype(np.float32)
    fw[0] = 0.0
    # soft posteriors + a frame with an all-zero target row (masked, nnet-loss.cc:80-85)
    tgt_soft = tgt.copy()
    tgt_soft[1] *= 0
    if rows > 2:
        tgt_soft[2] = 0
        tgt_soft[2, :2] = [0.25, 0.75]
    for t_np, use_labels in ((tgt, True), (tgt, False), (tgt_soft, False)):
        ref_diff, st = oracle.xent_eval(fw, y, t_np)
        yd = T(y, dev)
        diff = torch.empty_like(yd)
        stats = torch.zeros(5, dtype=torch.float64, device=dev)
        if use_labels:
            aslp.ops.xent_eval(yd, T(fw, dev), diff, stats, labels=T(labels, dev))
        else:
            aslp.ops.xent_eval(yd, T(fw, dev), diff, stats, targets=T(t_np, dev))
        assert oracle.rel_err(diff.cpu().numpy(), ref_diff) < 1e-6
        s = stats.cpu().numpy()
        ref = np.array([st["frames"], st["correct"], st["loss"], st["entropy"], st["likelyhood"]])
        assert np.allclose(s, ref, rtol=1e-5, atol=1e-6), (s, ref)


@pytest.mark.parametrize("rows,cols", [(20, 5), (1024, 2048), (129, 70), (0, 8)])
def test_add_row_sum_mat_vec(aslp, oracle, dev, rows, cols):
    rng = np.random.default_rng(8)
    M = rng.standard_normal((rows, cols)).astype(np.float32)
    v0 = rng.standard_normal(cols).astype(np.float32)
    v = T(v0, dev)
    aslp.ops.add_row_sum_mat_vec(0.43243, T(M, dev) if rows else torch.empty(0, cols, device=dev), 1.423, v)
    ref = 0.43243 * M.astype(np.float64).sum(0) + 1.423 * v0
    assert oracle.rel_err(v.cpu().numpy(), ref) < 1e-5


def test_aslp_group_ops(aslp, oracle, dev):
    """ASLP-added kernels, with the reference unit tests' shapes and expectations
    (cu-matrix-test.cc:1056-1123)."""
    rng = np.random.default_rng(9)
    rowsM, cols, P = 21, 6, 7
    M0 = rng.standard_normal((rowsM, cols)).astype(np.float32)
    A = rng.standard_normal((rowsM * P, cols)).astype(np.float32)
    Md, Ad = T(M0, dev), T(A, dev)
    aslp.lib.cudaF_add_row_sum_mat(aslp.Dim3(1, 1, 1), aslp.Dim3(1, 1, 1), aslp.ops.ptr(Md), aslp.ops.ptr(Ad), aslp.ops.dim(Md), cols, P, 0.43243, 1.423)
    aslp.check_error()
    ref = M0.copy()
    oracle.lib.orc_add_row_sum_mat(ref, cols, rowsM, cols, A, cols, rowsM * P, 0.43243, 1.423)
    assert oracle.rel_err(Md.cpu().numpy(), ref) < 1e-6
    check = 1.423 * M0 + 0.43243 * A.reshape(rowsM, P, cols).sum(1)  # "slow version" of the reference test
    assert oracle.rel_err(Md.cpu().numpy(), check) < 1e-5
    # AddConvMatMatElements: rowsA = 1000, rowsB = 8, alpha 1 beta 0
    rowsA, rowsB, cols = 1000, 8, 5
    A = rng.standard_normal((rowsA, cols)).astype(np.float32)
    B = rng.standard_normal((rowsB, cols)).astype(np.float32)
    rowsM = (rowsA - rowsB + 1) * rowsB
    Md = torch.full((rowsM, cols), float("nan"), device=dev)
    aslp.lib.cudaF_add_conv_mat_mat_elements(aslp.Dim3(1, 1, 1), aslp.Dim3(2, rowsB, 1), aslp.ops.ptr(Md), aslp.ops.ptr(T(A, dev)), aslp.ops.ptr(T(B, dev)),
                                             aslp.ops.dim(Md), cols, cols, 1.0, 0.0)
    aslp.check_error()
    ref = np.zeros((rowsM, cols), np.float32)
    oracle.lib.orc_add_conv_mat_mat_elements(ref, cols, cols, A, cols, rowsA, B, cols, rowsB, 1.0, 0.0)
    assert np.array_equal(Md.cpu().numpy(), ref)


@pytest.mark.parametrize("rows,C,cifg", [(1536, 320, False), (37, 20, False), (100, 65, True), (1, 4, False), (3000, 1024, False)])
@pytest.mark.parametrize("clip,lr", [(0.0, 0.0), (0.7, 0.01)])
def test_rnn_vec_grads(aslp, oracle, dev, rows, C, cifg, clip, lr):
    """bias / peephole gradients of one LSTM direction in one launch (lc.h:1005-1058, :1092-1104) vs float64 numpy"""
    rng = np.random.default_rng(rows + C)
    G = 3 if cifg else 4
    width = (G + 3) * C + 8
    d = T(rng.standard_normal((rows, width)).astype(np.float32), dev)
    y = T(rng.standard_normal((rows + 2, width)).astype(np.float32), dev)
    mmt = 0.9
    names = ["bias"] + ([] if cifg else ["pi"]) + ["pf", "po"]
    off = {"bias": 0, "pi": C, "pf": C if cifg else 2 * C, "po": 2 * C if cifg else 3 * C}
    n = {"bias": G * C, "pi": C, "pf": C, "po": C}
    xrow = {"bias": None, "pi": 0, "pf": 0, "po": 1}
    corr0 = {k: rng.standard_normal(n[k]).astype(np.float32) for k in names}
    par0 = {k: rng.standard_normal(n[k]).astype(np.float32) for k in names}
    corr = {k: T(corr0[k], dev) for k in names}
    par = {k: T(par0[k], dev) for k in names}
    jobs = []
    for k in names:
        dv = d[:, off[k]:off[k] + n[k]]
        xv = None if xrow[k] is None else y[xrow[k]:xrow[k] + rows, G * C:G * C + C]
        jobs.append((dv, xv, corr[k], par[k]))
    # a job list longer than one launch carries (8): the same jobs three times over, on copies of their buffers
    extra = [(dv, xv, c.clone(), q.clone()) for _ in range(2) for (dv, xv, c, q) in jobs]
    aslp.ops.rnn_vec_grads(jobs + extra, d.stride(0), rows, mmt, clip, -lr)
    torch.cuda.synchronize()
    for i, (dv, xv, c, q) in enumerate(extra):
        assert torch.equal(c, jobs[i % len(jobs)][2]) and torch.equal(q, jobs[i % len(jobs)][3]), i
    dn, yn = d.cpu().numpy().astype(np.float64), y.cpu().numpy().astype(np.float64)
    for k in names:
        g = dn[:, off[k]:off[k] + n[k]]
        if xrow[k] is not None:
            g = g * yn[xrow[k]:xrow[k] + rows, G * C:G * C + C]
        ref = g.sum(0) + mmt * corr0[k]
        if clip > 0:
            ref = np.clip(ref, -clip, clip)
        assert oracle.rel_err(corr[k].cpu().numpy(), ref) < 1e-5, k
        assert oracle.rel_err(par[k].cpu().numpy(), par0[k] - lr * ref) < 1e-5, k


@pytest.mark.parametrize("rows,cols", [(256, 128), (1024, 2048), (129, 260)])
def test_bn_backward_with_folded_sigmoid_is_bit_identical(aslp, dev, rows, cols):
    """aslp_bn_backward_act forming dy = od * y * (1 - y) on the fly must give, bit for bit, what Sigmoid's backward followed by
    the plain BatchNormalization backward gives (the folded and unfolded executors rely on it): the products are rounded on
    their own in both, never contracted into the column sums.  Panel-resident and three-launch paths."""
    g = torch.Generator(device="cpu").manual_seed(1)
    od = torch.randn(rows, cols, generator=g).to(dev)
    xhat = torch.randn(rows, cols, generator=g).to(dev)
    y = torch.sigmoid(torch.randn(rows, cols, generator=g)).to(dev)
    scale = (torch.rand(cols, generator=g) + 0.5).to(dev)
    inv = (torch.rand(cols, generator=g) + 0.5).to(dev)
    ptr, dim, lib = aslp.ops.ptr, aslp.ops.dim, aslp.ops.lib
    res = []
    for folded in (True, False):
        xh, ds, dsh = xhat.clone(), torch.zeros(cols, device=dev), torch.zeros(cols, device=dev)
        ind = torch.empty(rows, cols, device=dev)
        if folded:
            lib.aslp_bn_backward_act(None, dim(od), ptr(od), dim(od).stride, ptr(xh), dim(xh).stride, ptr(scale), None, ptr(inv), ptr(ds), ptr(dsh), 0.0,
                                     ptr(ind), dim(ind).stride, ptr(y), dim(y).stride)
        else:
            d = torch.empty_like(od)
            aslp.ops.diff_sigmoid(d, y, od)
            lib.aslp_bn_backward_act(None, dim(d), ptr(d), dim(d).stride, ptr(xh), dim(xh).stride, ptr(scale), None, ptr(inv), ptr(ds), ptr(dsh), 0.0,
                                     ptr(ind), dim(ind).stride, None, 0)
        aslp.ops.check_error()
        torch.cuda.synchronize()
        res.append([t.cpu().numpy() for t in (ds, dsh, ind, xh)])
    for name, a, b in zip(("dscale", "dshift", "in_diff", "xhat <- dy * gamma"), res[0], res[1]):
        assert np.array_equal(a, b), name


@pytest.mark.parametrize("rows,cols,softmax", [(1024, 3000, 1), (1024, 3000, 0), (257, 600, 1), (64, 9000, 0)])
def test_xent_deferred_row_sums_are_bit_identical(aslp, dev, rows, cols, softmax):
    """aslp_xent_eval_rows + one aslp_xent_sum_rowstats over several batches = one aslp_xent_eval_p per batch: the same diff and the same
    bits in the five accumulators (Xent keeps the per-row statistics of up to 32 steps and adds them up when Report() wants them)."""
    ptr, dim, lib = aslp.ops.ptr, aslp.ops.dim, aslp.ops.lib
    g = torch.Generator(device=dev).manual_seed(rows * 3 + cols)
    nb = 7
    acts = [torch.randn(rows, cols, device=dev, generator=g) * 3 for _ in range(nb)]
    if not softmax:
        acts = [torch.softmax(a, 1).contiguous() for a in acts]
    lab = [torch.randint(0, cols, (rows,), device=dev, generator=g, dtype=torch.int32) for _ in range(nb)]
    fw = [(torch.rand(rows, device=dev, generator=g) > 0.1).float() * 0.75 for _ in range(nb)]
    stats_a = torch.full((5,), 0.125, device=dev, dtype=torch.float64)
    stats_b = stats_a.clone()
    room = torch.empty(nb, rows, 5, device=dev, dtype=torch.float64)
    da, db = torch.empty(rows, cols, device=dev), torch.empty(rows, cols, device=dev)
    for b in range(nb):
        lib.aslp_xent_eval_p(ptr(acts[b]), dim(acts[b]), ptr(lab[b]), ptr(fw[b]), ptr(da), dim(da).stride, ptr(stats_a), softmax, None)
        lib.aslp_xent_eval_rows(ptr(acts[b]), dim(acts[b]), ptr(lab[b]), ptr(fw[b]), ptr(db), dim(db).stride, ptr(room[b]), softmax, None)
        aslp.ops.check_error()
        assert torch.equal(da, db), b
    lib.aslp_xent_sum_rowstats(ptr(room), rows, nb, ptr(stats_b))
    aslp.ops.check_error()
    torch.cuda.synchronize()
    assert torch.equal(stats_a, stats_b), (stats_a, stats_b)
    assert stats_a[0].item() > 0.125 and torch.isfinite(stats_a).all()


def test_copy_mat_trans(aslp, dev):
    """aslp_copy_mat_trans: dst = src^T, strided operands (what the recurrent layers use to refresh their K-contiguous weight copies)"""
    ptr, dim, lib = aslp.ops.ptr, aslp.ops.dim, aslp.ops.lib
    for rows, cols in ((512, 1024), (37, 5), (1, 9), (2048, 256), (33, 65), (64, 31)):   # (32 x 32 LDS tiles: whole, ragged and single-row grids)
        src = torch.randn(cols, rows + 3, device=dev)[:, :rows]      # [cols x rows], stride rows + 3
        dst = torch.full((rows, cols + 2), 9.0, device=dev)
        view = dst[:, :cols]
        MD = aslp._lib.MatrixDim(rows, cols, cols + 2)
        lib.aslp_copy_mat_trans(ptr(dst), MD, ptr(src), rows + 3)
        aslp.ops.check_error()
        torch.cuda.synchronize()
        assert torch.equal(view, src.t()) and bool((dst[:, cols:] == 9.0).all())


def _planes_to_host(aslp, po, rows, cols):
    """the [rows x cols] region of a PlanesOut's two fp16 planes, and the bound's bits"""
    memcpy = aslp.lib.hipMemcpy
    memcpy.restype = C.c_int
    memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = []
    for p in (po.hi, po.lo):
        h = np.empty((rows, po.ld), np.float16)
        assert memcpy(h.ctypes.data, p, 2 * rows * po.ld, 2) == 0
        assert not h[:, cols:].any()   # the padding columns stay zero
        out.append(h[:, :cols].copy())
    slot = np.empty(1, np.uint32)
    assert memcpy(slot.ctypes.data, po.slot, 4, 2) == 0
    return out[0], out[1], int(slot[0])


@pytest.mark.parametrize("rows,cols,with_dst", [(1024, 440, True), (1024, 440, False), (256, 40, True), (3000, 2048, True), (8, 4, True), (32768, 440, True)])
def test_copy_mat_planes(aslp, dev, rows, cols, with_dst):
    """aslp_copy_mat_planes: the copy and the planes (bound = the matrix maximum, found by the launch's workgroups among themselves) of
    one launch against aslp_copy_mat + the maximum pass + the conversion pass, bit for bit; inf / NaN elements do not set the scale;
    repeated launches; a matrix too large for one resident grid is declined (0) and nothing is written."""
    _lib = aslp._lib
    ptr, dim, lib = aslp.ops.ptr, aslp.ops.dim, aslp.ops.lib
    g = torch.Generator(device=dev).manual_seed(rows + cols)
    planes = C.c_void_p(lib.aslp_planes_new())
    lib.aslp_planes_reserve(planes, rows, cols)
    try:
        for it in range(3):
            src = torch.randn(rows, cols, device=dev, generator=g) * 10.0 ** (3 * it - 3)
            if it == 2 and rows > 8:
                src[3, 1], src[5, 2] = float("inf"), float("nan")
            dst = torch.full((rows, cols), -7.0, device=dev) if with_dst else None
            po = _lib.PlanesOut()
            lib.aslp_planes_as_output(planes, C.byref(po))
            rc = lib.aslp_copy_mat_planes(ptr(dst) if with_dst else None, dim(dst if with_dst else src), ptr(src), dim(src).stride, C.byref(po))
            aslp.ops.check_error()
            torch.cuda.synchronize()
            if rows * cols // 4 > 2 * 256 * 256 * 16:
                assert rc == 0 and po.planes_written == 0
                assert dst is None or bool((dst == -7.0).all())
                return
            assert rc == 1 and po.planes_written == 1
            if with_dst:
                assert torch.equal(dst.view(torch.int32), src.view(torch.int32))
            hi, lo, bits = _planes_to_host(aslp, po, rows, cols)
            lib.aslp_coop_convert(0)
            try:
                ref = aslp.ops.Planes(src)   # maximum pass + conversion pass
            finally:
                lib.aslp_coop_convert(1)
            one = aslp.ops.Planes(src)       # aslp_planes_convert on the single launch
            opo = _lib.PlanesOut()
            lib.aslp_planes_as_output(one.h, C.byref(opo))
            ohi, olo, obits = _planes_to_host(aslp, opo, rows, cols)
            assert obits == bits and np.array_equal(ohi.view(np.uint16), hi.view(np.uint16)) and np.array_equal(olo.view(np.uint16), lo.view(np.uint16)), it
            rpo = _lib.PlanesOut()
            lib.aslp_planes_as_output(ref.h, C.byref(rpo))
            rhi, rlo, rbits = _planes_to_host(aslp, rpo, rows, cols)
            assert bits == rbits, it
            assert np.array_equal(hi.view(np.uint16), rhi.view(np.uint16)) and np.array_equal(lo.view(np.uint16), rlo.view(np.uint16)), it
    finally:
        lib.aslp_planes_free(planes)


def test_grid_wide_kernels_stand_down_on_a_shared_device(aslp, dev):
    """aslp_device_shared(1) (several processes on this GPU; ShmComm sets it): launches whose workgroups wait for ALL workgroups of the launch
    are not used -- two of them half resident beside each other would never finish.  aslp_copy_mat_planes declines, the BatchNormalization
    backward leaves the per-workgroup maxima for a conversion pass instead of the planes."""
    _lib = aslp._lib
    ptr, dim, lib = aslp.ops.ptr, aslp.ops.dim, aslp.ops.lib
    rows, cols = 1024, 2048
    x = torch.randn(rows, cols, device=dev)
    planes = C.c_void_p(lib.aslp_planes_new())
    lib.aslp_planes_reserve(planes, rows, cols)
    lib.aslp_device_shared(1)
    try:
        po = _lib.PlanesOut()
        lib.aslp_planes_as_output(planes, C.byref(po))
        dst = torch.empty_like(x)
        assert lib.aslp_copy_mat_planes(ptr(dst), dim(dst), ptr(x), dim(x).stride, C.byref(po)) == 0 and po.planes_written == 0
        mean, inv = x.mean(0).contiguous(), (1.0 / torch.sqrt(x.var(0, unbiased=False) + 1e-7)).contiguous()
        od, scale, shift = torch.randn(rows, cols, device=dev), torch.ones(cols, device=dev), torch.zeros(cols, device=dev)
        ds, dsh, ind = torch.zeros(cols, device=dev), torch.zeros(cols, device=dev), torch.empty(rows, cols, device=dev)
        lib.aslp_bn_backward_step_p(dim(od), ptr(od), dim(od).stride, None, 0, ptr(scale), ptr(shift), ptr(inv), ptr(ds), ptr(dsh), 0.0, 0.001,
                                    ptr(ind), dim(ind).stride, None, 0, ptr(x), ptr(mean), C.byref(po))
        aslp.ops.check_error()
        torch.cuda.synchronize()
        assert po.planes_written == 0 and po.nparts > 0
        parts = np.empty(po.nparts, np.float32)
        memcpy = aslp.lib.hipMemcpy
        memcpy.restype, memcpy.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert memcpy(parts.ctypes.data, po.parts, 4 * po.nparts, 2) == 0
        assert parts.max() == ind.abs().max().item()
    finally:
        lib.aslp_device_shared(0)
        lib.aslp_planes_free(planes)


def test_grid_wide_kernels_stand_down_with_two_launching_threads(aslp, dev):
    """Two host threads of one process that both launch cooperative kernels (the sync workers' thread mode): the launches that wait for
    all their workgroups are not used while both are alive -- the same hazard as two processes on one GPU -- and come back when the
    second thread has ended."""
    import threading
    _lib = aslp._lib
    ptr, dim, lib = aslp.ops.ptr, aslp.ops.dim, aslp.ops.lib
    x = torch.randn(512, 256, device=dev)
    torch.cuda.synchronize()

    def convert():
        planes = C.c_void_p(lib.aslp_planes_new())
        lib.aslp_planes_reserve(planes, 512, 256)
        po = _lib.PlanesOut()
        lib.aslp_planes_as_output(planes, C.byref(po))
        rc = lib.aslp_copy_mat_planes(None, dim(x), ptr(x), dim(x).stride, C.byref(po))
        aslp.ops.check_error()
        torch.cuda.synchronize()
        lib.aslp_planes_free(planes)
        return rc

    assert convert() == 1
    seen, go, done = [], threading.Event(), threading.Event()

    def other():
        seen.append(convert())      # this thread's first cooperative launch: two launching threads from here on
        go.set()
        done.wait(60)

    t = threading.Thread(target=other)
    t.start()
    assert go.wait(60)
    try:
        assert seen == [0] and convert() == 0
    finally:
        done.set()
        t.join()
    assert convert() == 1


@pytest.mark.parametrize("rows,cols,with_y", [(1024, 2048, True), (1024, 2048, False), (1000, 1024, True), (256, 2048, True)])
def test_bn_backward_leaves_in_diff_planes(aslp, dev, rows, cols, with_y):
    """aslp_bn_backward_step_p with planes to fill: the launch's workgroups find the maximum of |in_diff| among themselves and write the
    two fp16 planes scaled by it -- bit for bit the planes (and the bound) the maximum pass + conversion pass make of the fp32 in_diff the same
    launch wrote.  Repeated launches (the exchange words carry a per-launch token and are never reset) and a launch without planes in
    between.  Shapes the cooperative kernel does not serve must say so (planes_written 0) and leave the maxima or nothing."""
    _lib = aslp._lib
    ptr, dim, lib = aslp.ops.ptr, aslp.ops.dim, aslp.ops.lib
    g = torch.Generator(device="cpu").manual_seed(rows + cols)
    x = torch.randn(rows, cols, generator=g).to(dev)
    mean, inv = x.mean(0).contiguous(), (1.0 / torch.sqrt(x.var(0, unbiased=False) + 1e-7)).contiguous()
    y = torch.sigmoid(torch.randn(rows, cols, generator=g)).to(dev) if with_y else None
    planes = C.c_void_p(lib.aslp_planes_new())
    lib.aslp_planes_reserve(planes, rows, cols)
    try:
        for it in range(4):
            od = (torch.randn(rows, cols, generator=g) * 10.0 ** (it - 2)).to(dev)
            scale, shift = (torch.rand(cols, generator=g) + 0.5).to(dev), torch.zeros(cols, device=dev)
            ds, dsh = torch.zeros(cols, device=dev), torch.zeros(cols, device=dev)
            ind = torch.empty(rows, cols, device=dev)
            po = _lib.PlanesOut()
            if it != 2:
                lib.aslp_planes_as_output(planes, C.byref(po))
            lib.aslp_bn_backward_step_p(dim(od), ptr(od), dim(od).stride, None, 0, ptr(scale), ptr(shift), ptr(inv), ptr(ds), ptr(dsh), 0.0, 0.001,
                                        ptr(ind), dim(ind).stride, ptr(y) if with_y else None, dim(y).stride if with_y else 0, ptr(x), ptr(mean),
                                        C.byref(po))
            aslp.ops.check_error()
            torch.cuda.synchronize()
            if it == 2:
                assert po.planes_written == 0
                continue
            if not po.planes_written:
                pytest.skip("this shape is not served by the cooperative kernel")
            assert po.nparts == 0
            hi, lo, bits = _planes_to_host(aslp, po, rows, cols)
            lib.aslp_coop_convert(0)
            try:
                ref = aslp.ops.Planes(ind)   # maximum pass + conversion pass over the fp32 in_diff
            finally:
                lib.aslp_coop_convert(1)
            rpo = _lib.PlanesOut()
            lib.aslp_planes_as_output(ref.h, C.byref(rpo))
            rhi, rlo, rbits = _planes_to_host(aslp, rpo, rows, cols)
            assert bits == rbits and np.float32(ind.abs().max().item()).view(np.uint32) == bits, it
            assert np.array_equal(hi.view(np.uint16), rhi.view(np.uint16)) and np.array_equal(lo.view(np.uint16), rlo.view(np.uint16)), it
    finally:
        lib.aslp_planes_free(planes)


@pytest.mark.parametrize("tA,tB,M,N,K,mode", [
    (0, 1, 1920, 2048, 512, "bias"), (0, 1, 1920, 256, 512, "act_out"), (0, 0, 1920, 512, 256, "plain"), (0, 0, 1920, 256, 2048, "beta1"),
    (0, 0, 2048, 512, 256, "plain"), (1, 0, 2048, 512, 1920, "sgd"), (1, 0, 2048, 256, 1920, "sgd"), (1, 0, 256, 512, 1920, "sgd"),
    (1, 1, 96, 80, 64, "plain"), (0, 1, 33, 20, 18, "plain"), (0, 1, 64, 64, 30, "bias")])
def test_sgemm_pair_matches_two_products(aslp, dev, tA, tB, M, N, K, mode):
    """aslp_sgemm_pair_ex: the batched products of the two directions of a bidirectional recurrent layer (cfg3 shapes: x -> gates,
    m -> r with the second store, d_m, d_r, W_eff, the three weight gradients with momentum + clip + SGD step), one launch for both.
    Against float64 and against two single launches (equal up to the order of the K-split partial sums); the last shapes are not
    eligible for the paired kernel (K % 4, unaligned rows) and must come out of the two-launch fallback unchanged."""
    g = torch.Generator(device=dev).manual_seed(M * 7 + N * 3 + K)
    mk = lambda *s: torch.randn(*s, device=dev, generator=g)
    A = [mk(*((K, M) if tA else (M, K))) for _ in range(2)]
    B = [mk(*((N, K) if tB else (K, N))) for _ in range(2)]
    C0 = [mk(M, N) for _ in range(2)]
    W0 = [mk(M, N) for _ in range(2)]
    bias = [mk(N) for _ in range(2)]
    beta = {"beta1": 1.0, "sgd": 0.9}.get(mode, 0.0)

    def run(paired):
        Cs, Ws, acts = [c.clone() for c in C0], [w.clone() for w in W0], [torch.zeros(M, 2 * N, device=dev) for _ in range(2)]
        eps = []
        for i in range(2):
            if mode == "bias":
                eps.append(aslp._lib.GemmEpilogue(bias[i].data_ptr(), 0.0, None, 0, 0.0, None, 0, 0))
            elif mode == "act_out":   # second store into a column block of a wider matrix, like the LSTM's [r_f | r_b] output
                eps.append(aslp._lib.GemmEpilogue(None, 0.0, None, 0, 0.0, acts[0].data_ptr() + 4 * N * i, 2 * N, 0))
            elif mode == "sgd":
                eps.append(aslp._lib.GemmEpilogue(None, 50.0, Ws[i].data_ptr(), N, -0.01, None, 0, 0))
            else:
                eps.append(None)
        if paired:
            aslp.ops.sgemm_pair(tA, tB, 1.0, A[0], A[1], B[0], B[1], beta, Cs[0], Cs[1], eps[0], eps[1])
        else:
            for i in range(2):
                aslp.ops.sgemm(tA, tB, 1.0, A[i], B[i], beta, Cs[i], eps[i])
        return Cs, Ws, acts

    (Cp, Wp, actp), (Cs, Ws, acts) = run(True), run(False)
    rel = lambda x, r: ((x.double() - r.double()).norm() / r.double().norm()).item()
    for i in range(2):
        ref = (A[i].t() if tA else A[i]).double() @ (B[i].t() if tB else B[i]).double() + beta * C0[i].double()
        if mode == "bias":
            ref = ref + bias[i].double()
        if mode == "sgd":
            ref = ref.clamp(-50.0, 50.0)
            assert rel(Wp[i], W0[i].double() - 0.01 * ref) < 2e-6
            assert rel(Wp[i], Ws[i]) < 1e-6
        assert rel(Cp[i], ref) < 2e-6, (i, rel(Cp[i], ref))
        assert rel(Cp[i], Cs[i]) < 1e-6
    if mode == "act_out":
        assert torch.equal(actp[0][:, :N], Cp[0]) and torch.equal(actp[0][:, N:], Cp[1])
    # run-to-run reproducible
    Cp2, Wp2, _ = run(True)
    assert all(torch.equal(x, y) for x, y in zip(Cp + Wp, Cp2 + Wp2))


@pytest.mark.parametrize("M,N,K,force", [(1024, 2048, 440, 0), (1024, 2048, 2048, 212), (1000, 96, 64, 0), (77, 40, 36, 0), (256, 128, 130, 0), (1024, 2048, 512, 7)])
def test_gemm_column_statistics_feed_batchnorm(aslp, dev, M, N, K, force):
    """aslp_gemm_epilogue.colstats: the forward product x = in W^T + b also leaves, per 32-row group and column, sum x, sum (float)(x*x)
    and sum x*x in double -- from the LDS-DMA kernels' epilogue, from one extra pass for the other kernels (odd K, forced
    register-staged tile) -- and aslp_bn_forward_stats normalises from those partials without a statistics pass of its own.
    The partials against float64 sums of the stored output; the normalisation (+ folded Sigmoid, running accumulators) against
    aslp_bn_forward_act on the same matrix."""
    from kaldi_aslp_amd._lib import GemmEpilogue
    import ctypes as C
    g = torch.Generator(device=dev).manual_seed(M + N + K)
    A = torch.randn(M, K, device=dev, generator=g)
    W = torch.randn(N, K, device=dev, generator=g) * 0.1
    b = torch.randn(N, device=dev, generator=g)
    groups, ld = (M + 31) // 32, (N + 3) & ~3
    stats = torch.full((3, groups, ld), float("nan"), dtype=torch.float64, device=dev)
    x = torch.empty(M, N, device=dev)
    ep = GemmEpilogue(b.data_ptr(), 0.0, None, 0, 0.0, None, 0, 0, None, 0.0, None, 0.0, stats.data_ptr(), ld)
    aslp.lib.aslp_gemm_force_tile(force)
    try:
        aslp.ops.sgemm(0, 1, 1.0, A, W, 0.0, x, ep)
    finally:
        aslp.lib.aslp_gemm_force_tile(0)
    xp = torch.zeros(groups * 32, N, dtype=torch.float64, device=dev)
    xp[:M] = x.double()
    xg = xp.view(groups, 32, N)
    assert torch.allclose(stats[0, :, :N], xg.sum(1), rtol=1e-12, atol=1e-9)
    assert torch.allclose(stats[2, :, :N], (xg * xg).sum(1), rtol=1e-12, atol=1e-9)
    x32 = torch.zeros(groups * 32, N, device=dev)
    x32[:M] = x
    assert torch.allclose(stats[1, :, :N], (x32 * x32).double().view(groups, 32, N).sum(1), rtol=1e-12, atol=1e-9)
    # the BatchNormalization that consumes them
    scale, shift = torch.rand(N, device=dev, generator=g) + 0.5, torch.randn(N, device=dev, generator=g)
    outs = []
    for from_stats in (True, False):
        out, act = torch.empty(M, N, device=dev), torch.empty(M, N, device=dev)
        mean, inv = torch.empty(N, device=dev), torch.empty(N, device=dev)
        accm = torch.ones(N, dtype=torch.float64, device=dev)
        accv = torch.ones(N, dtype=torch.float64, device=dev)
        d = aslp.ops.dim(x)
        if from_stats:
            ran = aslp.lib.aslp_bn_forward_stats(x.data_ptr(), d, out.data_ptr(), N, scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), inv.data_ptr(),
                                                 accm.data_ptr(), accv.data_ptr(), 1e-7, act.data_ptr(), N, stats.data_ptr(), groups, ld)
            aslp._lib.check_error()
            served = N % 32 == 0 and M <= 1024
            assert bool(ran) == served, (ran, served)
            if not ran:
                return
        else:
            aslp.lib.aslp_bn_forward_act(x.data_ptr(), d, out.data_ptr(), N, None, 0, scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), inv.data_ptr(),
                                         accm.data_ptr(), accv.data_ptr(), 1e-7, act.data_ptr(), N)
            aslp._lib.check_error()
        outs.append((out, act, mean, inv, accm, accv))
    for a, r in zip(outs[0], outs[1]):
        assert torch.allclose(a, r, rtol=2e-6, atol=1e-6), (a - r).abs().max()


@pytest.mark.parametrize("tA,tB,M,N,K,force", [(0, 0, 1920, 256, 2048, 0), (0, 1, 100, 72, 64, 0), (1, 0, 256, 512, 1920, 0), (0, 0, 130, 44, 36, 0), (0, 1, 512, 256, 128, 7)])
def test_sgemm_beta_term_from_another_matrix(aslp, dev, tA, tB, M, N, K, force):
    """aslp_gemm_epilogue.c_src: C = alpha op(A) op(B) + beta * c_src (the LSTM's d_r = out_diff + dGATES(next) W_r without the copy of
    out_diff into d_r first).  Same bits as copying c_src into C and running the classic form; LDS-DMA kernels (with and without a K
    split), the unaligned fallback and a forced register-staged tile."""
    from kaldi_aslp_amd._lib import GemmEpilogue
    g = torch.Generator(device=dev).manual_seed(M + N * 3 + K)
    A = torch.randn((K, M) if tA else (M, K), device=dev, generator=g)
    B = torch.randn((N, K) if tB else (K, N), device=dev, generator=g)
    wide = torch.randn(M, 2 * N + 4, device=dev, generator=g)
    src = wide[:, N + 4:]            # a column block of a wider matrix, like out_diff's backward-direction half
    want = src.clone()
    got = torch.full((M, N), float("nan"), device=dev)
    ep = GemmEpilogue(None, 0.0, None, 0, 0.0, None, 0, 0, None, 0.0, None, 0.0, None, 0, src.data_ptr(), wide.stride(0))
    aslp.lib.aslp_gemm_force_tile(force)
    try:
        aslp.ops.sgemm(tA, tB, 0.5, A, B, 0.75, got, ep)
        aslp.ops.sgemm(tA, tB, 0.5, A, B, 0.75, want)
    finally:
        aslp.lib.aslp_gemm_force_tile(0)
    assert torch.equal(got, want)
    ref = 0.5 * ((A.t() if tA else A).double() @ (B.t() if tB else B).double()) + 0.75 * src.double()
    assert ((got.double() - ref).norm() / ref.norm()).item() < 2e-6


def test_grid_wide_kernels_stand_down_beside_a_thread_of_persistent_recurrences(aslp, dev):
    """a host thread that only ever launches persistent recurrences (GruStreams here) never came through the cooperative
    kernels' own registration, so another thread's grid-wide launch could sit half placed beside its persistent grid.  The launchers of
    the recurrences now register in the same count: while that thread lives the grid-wide launches of THIS thread are not used; DNN +
    BatchNormalization steps on this thread and GRU steps on the other, side by side, finish without a hand-off time-out and give the bits
    of the same steps run alone."""
    import threading
    _lib = aslp._lib
    ptr, dim, lib = aslp.ops.ptr, aslp.ops.dim, aslp.ops.lib
    x = torch.randn(512, 256, device=dev)
    S, T, H, A = 8, 12, 128, 16
    gru_proto = ("<NnetProto>\n<GruStreams> <InputDim> %d <OutputDim> %d <ParamScale> 0.1 <ClipGradient> 5.0\n"
                 "<AffineTransform> <InputDim> %d <OutputDim> %d <BiasMean> 0.0 <BiasRange> 0.0 <ParamStddev> 0.1\n<Softmax> <InputDim> %d <OutputDim> %d\n</NnetProto>\n"
                 % (H, H, H, A, A, A))
    dnn_proto = ("<NnetProto>\n<AffineTransform> <InputDim> 256 <OutputDim> 512 <BiasMean> -2.0 <BiasRange> 4.0 <ParamStddev> 0.1\n"
                 "<BatchNormalization> <InputDim> 512 <OutputDim> 512\n<Sigmoid> <InputDim> 512 <OutputDim> 512\n"
                 "<AffineTransform> <InputDim> 512 <OutputDim> 64 <BiasMean> 0.0 <BiasRange> 0.0 <ParamStddev> 0.1\n<Softmax> <InputDim> 64 <OutputDim> 64\n</NnetProto>\n")
    g = torch.Generator(device=dev).manual_seed(9)
    xg = torch.randn(T * S, H, device=dev, generator=g)
    lg = torch.randint(0, A, (T * S,), device=dev, generator=g, dtype=torch.int32)
    ld = torch.randint(0, 64, (512,), device=dev, generator=g, dtype=torch.int32)
    torch.cuda.synchronize()

    def convert():
        planes = C.c_void_p(lib.aslp_planes_new())
        lib.aslp_planes_reserve(planes, 512, 256)
        po = _lib.PlanesOut()
        lib.aslp_planes_as_output(planes, C.byref(po))
        rc = lib.aslp_copy_mat_planes(None, dim(x), ptr(x), dim(x).stride, C.byref(po))
        aslp.ops.check_error()
        torch.cuda.synchronize()
        lib.aslp_planes_free(planes)
        return rc

    # (nets are made one after the other on this thread: Nnet::Init draws from the process-wide generator, as the reference's does from rand())
    def gru_net():
        net = aslp.Nnet.Init(gru_proto, seed=3)
        net.SetTrainOptions(learn_rate=1e-3, momentum=0.0)
        net.SetSeqLengths([T] * S)
        return net

    def dnn_net():
        net = aslp.Nnet.Init(dnn_proto, seed=4)
        net.SetTrainOptions(learn_rate=1e-3, momentum=0.0)
        return net

    def gru_steps(net, n):
        xe = aslp.Xent()
        for i in range(n):
            net.ResetLstmStreams([1] * S)
            net.TrainStepXent(xe, xg, lg)
        torch.cuda.synchronize()
        return net.GetParams()

    def dnn_steps(net, n):
        xe = aslp.Xent()
        for i in range(n):
            net.TrainStepXent(xe, x, ld)
        torch.cuda.synchronize()
        return net.GetParams()

    n = 40
    ref_dnn = dnn_steps(dnn_net(), n)          # alone (this thread may use the grid-wide launches)
    ref_gru = gru_steps(gru_net(), n)
    assert convert() == 1
    nets = {"g1": gru_net(), "g": gru_net(), "d": dnn_net()}
    out, go, done, errs = {}, threading.Event(), threading.Event(), []

    def other():
        try:
            aslp.ops.use_torch_stream()
            gru_steps(nets["g1"], 1)            # this thread's first persistent launch: two grid-wide launchers from here on
            go.set()
            done.wait(120)
            out["gru"] = gru_steps(nets["g"], n)
        except Exception as e:   # noqa: BLE001
            errs.append(e)
            go.set()

    t = threading.Thread(target=other)
    t.start()
    assert go.wait(120) and not errs, errs
    try:
        assert convert() == 0                       # stands down although the other thread never launched a cooperative kernel
    finally:
        done.set()
    beside = dnn_steps(nets["d"], n)                # ... while the other thread runs its recurrences
    t.join()
    assert not errs, errs
    aslp.ops.check_error()                          # no hand-off time-out anywhere
    # beside the other thread the multi-launch paths run: they form the same values from the same maxima -- the same bits
    assert np.array_equal(beside, ref_dnn)
    assert np.array_equal(out["gru"], ref_gru)
    assert convert() == 1                           # the thread has ended: grid-wide launches are back
