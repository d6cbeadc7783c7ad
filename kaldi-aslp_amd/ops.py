"""torch.Tensor wrappers over the kernel C ABI (B1/B2).  Tensors must live on the GPU; the
wrappers only extract (pointer, rows, cols, stride) -- all arithmetic happens in
libaslp_hip.so.  Used by tests/, bench.py and the Python mirror of the sync workers."""
import contextlib
import ctypes as C

import torch

from ._lib import lib, MatrixDim, Dim3, GemmEpilogue, CtcComputeInfo, D3, PlanesOut, check_error


def _chk(t, dtype=torch.float32):
    if not t.is_cuda:
        raise RuntimeError("aslp ops need device tensors (no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError("expected %s, got %s" % (dtype, t.dtype))
    if t.dim() == 2 and t.stride(1) != 1:
        raise ValueError("matrix must be row-major with unit column stride")
    return t


def dim(t):
    """MatrixDim of a 2-D row-major tensor (or view with stride >= cols)."""
    if t.dim() == 1:
        return MatrixDim(1, t.shape[0], t.shape[0])
    return MatrixDim(t.shape[0], t.shape[1], t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1]))


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def use_torch_stream():
    """Enqueue library kernels on torch's current stream (so torch.cuda.Event sees them)."""
    lib.aslp_set_stream(C.c_void_p(torch.cuda.current_stream().cuda_stream))


def sgemm(transA, transB, alpha, A, B, beta, Cm, epilogue=None):
    """C = alpha*op(A)*op(B) + beta*C (cu-matrix.cc:1027-1061 semantics)."""
    _chk(A), _chk(B), _chk(Cm)
    M, N = Cm.shape
    K = A.shape[0] if transA else A.shape[1]
    ep = C.byref(epilogue) if epilogue is not None else None
    rc = lib.aslp_sgemm_ex(int(transA), int(transB), M, N, K, alpha, ptr(A), dim(A).stride, ptr(B), dim(B).stride,
                           beta, ptr(Cm), dim(Cm).stride, ep)
    if rc != 0:
        raise ValueError("aslp_sgemm argument error %d" % rc)
    check_error()


def set_operand_planes(n):
    """planes the layer products read per operand (aslp_gemm_operand_planes): 2 = hi and lo (fp32-equivalent operands), 1 = hi alone
    (fp16 operands, fp32 accumulation), -1 = what ASLP_GEMM_PLANES said"""
    lib.aslp_gemm_operand_planes(int(n))


@contextlib.contextmanager
def operand_planes(n):
    """products inside the block read n planes per operand; the mode in force before comes back on exit (as an explicit setting: where that
    mode was the environment's, the same value is now pinned -- the environment is read once per process, so nothing changes by it;
    set_operand_planes(-1) hands the choice back)"""
    before = lib.aslp_gemm_operand_planes_get()
    lib.aslp_gemm_operand_planes(int(n))
    try:
        yield
    finally:
        lib.aslp_gemm_operand_planes(before)


def set_split16_ragged(on):
    """split-fp16 layer products at sizes that are no multiple of 4 (aslp_gemm_split16_ragged): 1 = served (M, N >= 128 and K >= 64 remain),
    0 = refused as shipped (default), -1 = what ASLP_GEMM_S16_RAGGED said"""
    lib.aslp_gemm_split16_ragged(int(on))


@contextlib.contextmanager
def split16_ragged(on):
    """products and conversions inside the block run with the switch at `on`; the setting in force before comes back on exit (pinned as an
    explicit setting, as operand_planes does; set_split16_ragged(-1) hands the choice back to the environment)"""
    before = lib.aslp_gemm_split16_ragged_get()
    lib.aslp_gemm_split16_ragged(int(on))
    try:
        yield
    finally:
        lib.aslp_gemm_split16_ragged(before)


def set_lstm_operand_pieces(n):
    """fp16 pieces per operand inside the persistent LSTM recurrences (aslp_lstm_operand_pieces): 2 = hi and lo' (fp32-equivalent operands),
    1 = hi alone (fp16 operands, fp32 accumulation), -1 = what ASLP_LSTM_PIECES said"""
    lib.aslp_lstm_operand_pieces(int(n))


@contextlib.contextmanager
def lstm_operand_pieces(n):
    """persistent LSTM recurrences inside the block multiply with n pieces per operand; the mode in force before comes back on exit (pinned as
    an explicit setting, as operand_planes does; set_lstm_operand_pieces(-1) hands the choice back to the environment)"""
    before = lib.aslp_lstm_operand_pieces_get()
    lib.aslp_lstm_operand_pieces(int(n))
    try:
        yield
    finally:
        lib.aslp_lstm_operand_pieces(before)


def set_gru_seq_pieces(n):
    """fp16 pieces per operand of the products inside the persistent GRU recurrences (aslp_gru_seq_pieces): 0 = the fp32 instruction (default),
    2 = hi and lo' on the fp16 instruction (fp32-equivalent operands), 1 = hi alone (fp16 operands, fp32 accumulation), -1 = what
    ASLP_GRU_SEQ_PIECES said"""
    lib.aslp_gru_seq_pieces(int(n))


@contextlib.contextmanager
def gru_seq_pieces(n):
    """persistent GRU recurrences inside the block multiply with n pieces per operand (0 = the fp32 instruction); the setting in force before
    comes back on exit (pinned as an explicit setting, as lstm_operand_pieces does; set_gru_seq_pieces(-1) hands the choice back to the
    environment)"""
    before = lib.aslp_gru_seq_pieces_get()
    lib.aslp_gru_seq_pieces(int(n))
    try:
        yield
    finally:
        lib.aslp_gru_seq_pieces(before)


def set_lstm_step_split16(on):
    """split-fp16 products on the per-timestep LSTM path (aslp_lstm_step_split16): 1 = the step kernels multiply on the fp16 instruction with
    lstm_operand_pieces pieces per operand, 0 = the fp32 instruction (default), -1 = what ASLP_LSTM_STEP_SPLIT_F16 said"""
    lib.aslp_lstm_step_split16(int(on))


@contextlib.contextmanager
def lstm_step_split16(on):
    """per-timestep LSTM recurrences inside the block run with the switch at `on`; the setting in force before comes back on exit (pinned as an
    explicit setting, as lstm_operand_pieces does; set_lstm_step_split16(-1) hands the choice back to the environment)"""
    before = lib.aslp_lstm_step_split16_get()
    lib.aslp_lstm_step_split16(int(on))
    try:
        yield
    finally:
        lib.aslp_lstm_step_split16(before)


def set_gru_step_pieces(n):
    """fp16 pieces per operand of the four products of the per-timestep GRU path (aslp_gru_step_pieces): 0 = the fp32 instruction (default),
    2 = hi and lo' on the fp16 instruction (fp32-equivalent operands), 1 = hi alone (fp16 operands, fp32 accumulation), -1 = what
    ASLP_GRU_STEP_PIECES said"""
    lib.aslp_gru_step_pieces(int(n))


@contextlib.contextmanager
def gru_step_pieces(n):
    """per-timestep GRU recurrences inside the block multiply with n pieces per operand (0 = the fp32 instruction); the setting in force before
    comes back on exit (pinned as an explicit setting, as gru_seq_pieces does; set_gru_step_pieces(-1) hands the choice back to the
    environment)"""
    before = lib.aslp_gru_step_pieces_get()
    lib.aslp_gru_step_pieces(int(n))
    try:
        yield
    finally:
        lib.aslp_gru_step_pieces(before)


def set_fp16_operands(on):
    """the one switch for fp16 operands (aslp_fp16_operands): 1 = every product site that is faster with one fp16 piece per operand takes it
    by default (layer products, persistent and per-timestep LSTM recurrences, per-timestep GRU recurrences; the persistent GRU recurrences stay
    on the fp32 instruction), 0 = off (default),
    -1 = what ASLP_FP16_OPERANDS said.  Every site's own setter and environment variable still wins."""
    lib.aslp_fp16_operands(int(on))


@contextlib.contextmanager
def fp16_operands(on):
    """the umbrella switch at `on` inside the block; the state in force before comes back on exit (pinned as an explicit setting;
    set_fp16_operands(-1) hands the choice back to the environment)"""
    before = lib.aslp_fp16_operands_get()
    lib.aslp_fp16_operands(int(on))
    try:
        yield
    finally:
        lib.aslp_fp16_operands(before)


class Planes:
    """the two fp16 planes of an fp32 matrix (aslp_planes_*): made once, read by every product the matrix takes part in"""

    def __init__(self, t):
        self.h = C.c_void_p(lib.aslp_planes_new())
        self.t = _chk(t)
        rc = lib.aslp_planes_convert(self.h, ptr(t), dim(t))
        if rc != 0:
            raise ValueError("aslp_planes_convert error %d" % rc)
        check_error()

    def __del__(self):
        if getattr(self, "h", None):
            lib.aslp_planes_free(self.h)
            self.h = None


def sgemm_planes(transA, transB, alpha, A, pa, B, pb, beta, Cm, epilogue=None):
    """sgemm with prepared planes of A and / or B (Planes or None)"""
    _chk(A), _chk(B), _chk(Cm)
    M, N = Cm.shape
    K = A.shape[0] if transA else A.shape[1]
    ep = C.byref(epilogue) if epilogue is not None else None
    rc = lib.aslp_sgemm_planes_ex(int(transA), int(transB), M, N, K, alpha, ptr(A), dim(A).stride, pa.h if pa else None, ptr(B), dim(B).stride,
                                  pb.h if pb else None, beta, ptr(Cm), dim(Cm).stride, ep)
    if rc != 0:
        raise ValueError("aslp_sgemm_planes argument error %d" % rc)
    check_error()


def sgemm_pair(transA, transB, alpha, A0, A1, B0, B1, beta, C0, C1, ep0=None, ep1=None):
    """two products of one shape in one launch (aslp_sgemm_pair_ex)"""
    for t in (A0, A1, B0, B1, C0, C1):
        _chk(t)
    assert A0.shape == A1.shape and B0.shape == B1.shape and C0.shape == C1.shape
    assert dim(A0).stride == dim(A1).stride and dim(B0).stride == dim(B1).stride and dim(C0).stride == dim(C1).stride
    M, N = C0.shape
    K = A0.shape[0] if transA else A0.shape[1]
    rc = lib.aslp_sgemm_pair_ex(int(transA), int(transB), M, N, K, alpha, ptr(A0), ptr(A1), dim(A0).stride, ptr(B0), ptr(B1), dim(B0).stride,
                                beta, ptr(C0), ptr(C1), dim(C0).stride, C.byref(ep0) if ep0 is not None else None,
                                C.byref(ep1) if ep1 is not None else None)
    if rc != 0:
        raise ValueError("aslp_sgemm_pair argument error %d" % rc)
    check_error()


def sigmoid(y, x):
    lib.cudaF_sigmoid(D3, D3, ptr(_chk(y)), ptr(_chk(x)), dim(y), dim(x).stride); check_error()


def tanh(y, x):
    lib.cudaF_tanh(D3, D3, ptr(_chk(y)), ptr(_chk(x)), dim(y), dim(x).stride); check_error()


def diff_sigmoid(eout, y, e):
    lib.cudaF_diff_sigmoid(D3, D3, ptr(_chk(eout)), ptr(_chk(e)), ptr(_chk(y)), dim(eout), dim(e).stride, dim(y).stride); check_error()


def diff_tanh(eout, y, e):
    lib.cudaF_diff_tanh(D3, D3, ptr(_chk(eout)), ptr(_chk(e)), ptr(_chk(y)), dim(eout), dim(e).stride, dim(y).stride); check_error()


def diff_relu(in_diff, x, od):
    """in_diff = heaviside(x) * od, x the PRE-activation (aslp_diff_relu)"""
    lib.aslp_diff_relu(ptr(_chk(in_diff)), ptr(_chk(x)), ptr(_chk(od)), dim(in_diff), dim(x).stride, dim(od).stride); check_error()


def diff_sigmoid_p(eout, y, e, e_max_parts, planes_out):
    """diff_sigmoid which also leaves the fp16 planes of eout in planes_out (a _lib.PlanesOut), scaled by max(e_max_parts) / 4; 1 = planes
    written, 0 = eout alone"""
    rc = lib.aslp_diff_sigmoid_p(ptr(_chk(eout)), ptr(_chk(e)), ptr(_chk(y)), dim(eout), dim(e).stride, dim(y).stride, ptr(_chk(e_max_parts)),
                                 e_max_parts.numel(), C.byref(planes_out))
    check_error()
    return rc


def diff_tanh_p(eout, y, e, e_max_parts, planes_out):
    """diff_tanh with the planes of eout, scaled by max(e_max_parts); 1 = eout and planes written, 0 = not served, nothing launched"""
    rc = lib.aslp_diff_tanh_p(ptr(_chk(eout)), ptr(_chk(e)), ptr(_chk(y)), dim(eout), dim(e).stride, dim(y).stride, ptr(_chk(e_max_parts)),
                              e_max_parts.numel(), C.byref(planes_out))
    check_error()
    return rc


def diff_relu_p(in_diff, x, od, od_max_parts, planes_out):
    """diff_relu with the planes of in_diff, scaled by max(od_max_parts); 1 = in_diff and planes written, 0 = not served, nothing launched"""
    rc = lib.aslp_diff_relu_p(ptr(_chk(in_diff)), ptr(_chk(x)), ptr(_chk(od)), dim(in_diff), dim(x).stride, dim(od).stride, ptr(_chk(od_max_parts)),
                              od_max_parts.numel(), C.byref(planes_out))
    check_error()
    return rc


def softmax(y, x):
    lib.cudaF_softmax_reduce(0, 0, ptr(_chk(y)), ptr(_chk(x)), dim(y), dim(x).stride); check_error()


def splice(y, x, offsets):
    lib.cudaF_splice(D3, D3, ptr(_chk(y)), ptr(_chk(x)), ptr(_chk(offsets, torch.int32)), dim(y), dim(x)); check_error()


def splice_backward(in_diff, out_diff, offsets):
    lib.aslp_splice_backward(ptr(_chk(in_diff)), dim(in_diff), ptr(_chk(out_diff)), dim(out_diff).stride,
                             ptr(_chk(offsets, torch.int32)), offsets.numel()); check_error()


def randomize(y, x, copy_from):
    d_out = dim(y); d_out.rows = copy_from.numel()
    d_in = dim(x); d_in.rows = copy_from.numel()
    lib.cudaF_randomize(D3, D3, ptr(_chk(y)), ptr(_chk(x)), ptr(_chk(copy_from, torch.int32)), d_out, d_in); check_error()


def find_row_max_id(m):
    out = torch.empty(m.shape[0], dtype=torch.int32, device=m.device)
    lib.aslp_find_row_max_id(ptr(_chk(m)), dim(m), ptr(out)); check_error()
    return out


def add_row_sum_mat_vec(alpha, M, beta, v):
    lib.aslp_add_row_sum_mat_vec(alpha, ptr(_chk(M)), dim(M), beta, ptr(_chk(v))); check_error()


def rnn_vec_grads(jobs, d_stride, rows, mmt, clip, neg_lr):
    """jobs: list of (d_view, x_view or None, corr, param); d_view / x_view are [rows x n] column blocks of pitched buffers."""
    from ._lib import RnnVecGrad
    arr = (RnnVecGrad * len(jobs))()
    for k, (d, x, corr, param) in enumerate(jobs):
        arr[k].d = ptr(d); arr[k].x = ptr(x) if x is not None else None
        arr[k].ldx = x.stride(0) if x is not None else 0
        arr[k].n = d.shape[1]; arr[k].corr = ptr(_chk(corr)); arr[k].param = ptr(_chk(param))
    lib.aslp_rnn_vec_grads(arr, len(jobs), d_stride, rows, mmt, clip, neg_lr); check_error()


def bn_forward(x, out, xhat, scale, shift, mean, inv_std, acc_means=None, acc_vars=None, var_floor=1e-7):
    lib.aslp_bn_forward(ptr(_chk(x)), dim(x), ptr(_chk(out)), dim(out).stride, ptr(_chk(xhat)), dim(xhat).stride,
                        ptr(scale), ptr(shift), ptr(mean), ptr(inv_std), ptr(acc_means), ptr(acc_vars), var_floor)
    check_error()


def bn_backward(x, dy, xhat, scale, mean, inv_std, dscale, dshift, momentum, in_diff):
    lib.aslp_bn_backward(ptr(_chk(x)), dim(x), ptr(_chk(dy)), dim(dy).stride, ptr(_chk(xhat)), dim(xhat).stride,
                         ptr(scale), ptr(mean), ptr(inv_std), ptr(dscale), ptr(dshift), momentum,
                         ptr(in_diff), dim(in_diff).stride if in_diff is not None else 0)
    check_error()


def xent_eval(net_out, frame_weights, diff, stats, targets=None, labels=None):
    lib.aslp_xent_eval(ptr(_chk(net_out)), dim(net_out), ptr(targets), dim(targets).stride if targets is not None else 0,
                       ptr(labels), ptr(_chk(frame_weights)), ptr(_chk(diff)), dim(diff).stride,
                       ptr(_chk(stats, torch.float64)))
    check_error()


def xent_eval_rows(net_out, frame_weights, diff, rowstats, labels, softmax=False):
    """aslp_xent_eval_rows: the loss diff and the batch's per-row statistics (rowstats [rows x 5] float64); the sums are taken later"""
    lib.aslp_xent_eval_rows(ptr(_chk(net_out)), dim(net_out), ptr(labels), ptr(_chk(frame_weights)), ptr(_chk(diff)), dim(diff).stride,
                            ptr(_chk(rowstats, torch.float64)), int(bool(softmax)), None)
    check_error()


def xent_sum_rowstats(rowstats, rows, batches, stats):
    """aslp_xent_sum_rowstats: `batches` blocks of `rows` per-row statistics added to the five accumulators, in order"""
    lib.aslp_xent_sum_rowstats(ptr(_chk(rowstats, torch.float64)), rows, batches, ptr(_chk(stats, torch.float64)))
    check_error()


def _xent_sparse(fn, inp, row_begin, cols, weights, frame_weights, diff, out, softmax, post_out):
    for m in (inp, weights, frame_weights, diff, post_out):
        if m is not None:
            _chk(m)
    for m in (row_begin, cols):
        if m is not None:
            _chk(m, torch.int32)
    if out is not None:
        _chk(out, torch.float64)
    d = dim(inp) if inp is not None else MatrixDim(0, 0, 0)
    return fn(ptr(inp), d, ptr(row_begin), ptr(cols), ptr(weights), ptr(frame_weights), ptr(diff), dim(diff).stride if diff is not None else 0,
              ptr(out), int(bool(softmax)), ptr(post_out), dim(post_out).stride if post_out is not None else 0)


def xent_sparse_eval(inp, row_begin, cols, weights, frame_weights, diff, stats, softmax=False, post_out=None):
    """aslp_xent_sparse_eval: Xent on soft targets given as CSR (row_begin int32 [rows + 1], cols int32 [nnz] strictly increasing within a
    row, weights [nnz]) in one launch, the five sums added to stats (float64 [5]).  softmax: `inp` holds the activations in front of the
    Softmax and post_out (optional) receives the posteriors.  Returns served; nothing raises, so that a refusal (served == 0, the error
    string set) can be looked at: the caller reads last_error() / check_error()."""
    return _xent_sparse(lib.aslp_xent_sparse_eval, inp, row_begin, cols, weights, frame_weights, diff, stats, softmax, post_out)


def xent_sparse_eval_rows(inp, row_begin, cols, weights, frame_weights, diff, rowstats, softmax=False, post_out=None):
    """aslp_xent_sparse_eval_rows: the same, the batch's per-row statistics left in rowstats (float64 [rows x 5]) for xent_sum_rowstats"""
    return _xent_sparse(lib.aslp_xent_sparse_eval_rows, inp, row_begin, cols, weights, frame_weights, diff, rowstats, softmax, post_out)


def set_xent_sparse(on):
    """A/B switch (ASLP_XENT_SPARSE=0): off = the engine's Xent::Eval on a Posterior that is not one-hot builds the dense target matrix and
    runs the dense kernel, as before; on (the default) = the posterior goes to the kernel as CSR.  Same bits either way."""
    lib.aslp_xent_sparse(int(bool(on)))


@contextlib.contextmanager
def xent_sparse(on):
    """the engine's evaluations inside the block run with the switch at `on`; the setting in force before comes back on exit"""
    before = lib.aslp_xent_sparse_get()
    lib.aslp_xent_sparse(int(bool(on)))
    try:
        yield
    finally:
        lib.aslp_xent_sparse(before)


def mse_eval(net_out, targets, frame_weights, diff, row_loss, scale=1.0, parts=None, frames_out=None):
    """aslp_mse_eval: diff = (net_out - targets) * w[row] (* scale), row_loss[row] (float64) = the row's sum of (e * e) * w[row]; parts
    (256 floats, optional) receives one maximum of the finite |diff| per workgroup.  Returns (served, nparts); nothing raises, so that a
    refusal (served == 0, the error string set) can be looked at: the caller reads last_error() / check_error()."""
    for m in (net_out, targets, frame_weights, diff):
        if m is not None:
            _chk(m)
    if row_loss is not None:
        _chk(row_loss, torch.float64)
    po = None
    if parts is not None:
        po = PlanesOut()
        po.parts = ptr(_chk(parts))
    d = dim(net_out) if net_out is not None else MatrixDim(0, 0, 0)
    args = (ptr(net_out), d, ptr(targets), dim(targets).stride if targets is not None else 0, ptr(frame_weights), float(scale), ptr(diff),
            dim(diff).stride if diff is not None else 0, ptr(row_loss), C.byref(po) if po is not None else None)
    if frames_out is not None:
        served = lib.aslp_mse_eval_w(*args, ptr(_chk(frames_out, torch.float64)))
    else:
        served = lib.aslp_mse_eval(*args)
    return served, (po.nparts if po is not None else 0)


def xent_blocks_eval(inp, blocks, labels, frame_weights, diff, softmax=True, mask=True, post_out=None, parts=None):
    """aslp_xent_blocks_eval: Xent over column blocks of `inp` in one launch.  blocks: a list of (offset, cols, weight, rowstats) with
    rowstats a float64 device tensor [rows x 5] (or None, to look at the refusal); labels int32 [rows x len(blocks)], relative to the
    block, < 0 = no target.  softmax: `inp` holds activations, else posteriors; mask: BlockSoftmax' backward on the diff; post_out
    (optional) receives the posteriors, parts (256 floats, optional) one maximum of the finite |diff| per workgroup.  Returns
    (served, nparts); nothing raises, so that a refusal (served == 0, the error string set) can be looked at."""
    from ._lib import XentBlock
    for m in (inp, frame_weights, diff, post_out):
        if m is not None:
            _chk(m)
    if labels is not None:
        _chk(labels, torch.int32)
    arr = (XentBlock * max(len(blocks), 1))()
    for k, (offset, cols, weight, rowstats) in enumerate(blocks):
        arr[k].offset, arr[k].cols, arr[k].weight = int(offset), int(cols), float(weight)
        arr[k].rowstats = ptr(_chk(rowstats, torch.float64)) if rowstats is not None else None
    po = None
    if parts is not None:
        po = PlanesOut()
        po.parts = ptr(_chk(parts))
    d = dim(inp) if inp is not None else MatrixDim(0, 0, 0)
    served = lib.aslp_xent_blocks_eval(ptr(inp), d, arr, len(blocks), ptr(labels), ptr(frame_weights), ptr(diff),
                                       dim(diff).stride if diff is not None else 0, int(bool(softmax)), int(bool(mask)), ptr(post_out),
                                       dim(post_out).stride if post_out is not None else 0, C.byref(po) if po is not None else None)
    return served, (po.nparts if po is not None else 0)


def multitask_fused(on):
    """A/B switch (ASLP_MULTITASK_FUSED=0): off = nnet.MultiTaskLoss.Eval / Nnet.train_step_multitask run the op sequence of the
    reference's MultiTaskLoss::Eval, no BlockSoftmax is left to the loss"""
    lib.aslp_multitask_fused(int(bool(on)))


def ctc_loss(acts, labels, input_lengths, want_grad=True):
    """compute_ctc_loss (warp-ctc/include/ctc.h:88-97) on device activations [(maxT*mb) x A] laid out (t, n, p).
    labels: list of int lists; returns (costs numpy[mb], grads tensor or None)."""
    import numpy as np
    _chk(acts)
    mb = len(labels)
    A = acts.shape[-1]
    flat = [int(v) for l in labels for v in l] or [0]
    flat_c = (C.c_int * len(flat))(*flat)
    lab_len = (C.c_int * mb)(*[len(l) for l in labels])
    in_len = (C.c_int * mb)(*[int(t) for t in input_lengths])
    info = CtcComputeInfo(1, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    sz = C.c_size_t()
    st = lib.get_workspace_size(lab_len, in_len, A, mb, info, C.byref(sz))
    if st != 0:
        raise RuntimeError("get_workspace_size: " + lib.ctcGetStatusString(st).decode())
    ws = torch.empty(sz.value, dtype=torch.uint8, device=acts.device)
    grads = torch.zeros_like(acts) if want_grad else None
    costs = (C.c_float * mb)()
    st = lib.compute_ctc_loss(ptr(acts), ptr(grads), flat_c, lab_len, in_len, A, mb, costs, ptr(ws), info)
    if st != 0:
        raise RuntimeError("compute_ctc_loss: " + lib.ctcGetStatusString(st).decode())
    check_error()
    return np.array(list(costs), np.float32), grads


def ctc_token_errors(acts, labels, input_lengths=None):
    """aslp_ctc_token_errors (include/aslp_ctc.h) on device activations [(maxT*mb) x A], row t * mb + n: per utterance the best path
    (argmax, first strict maximum; repeats collapsed; blanks dropped) and its edit distance to the labels.
    labels: list of int lists; input_lengths None: one sequence of all rows.  Returns (errors numpy[mb] int32, hyps list of int lists)."""
    import numpy as np
    _chk(acts)
    mb = len(labels)
    flat = [int(v) for l in labels for v in l] or [0]
    flat_c = (C.c_int * len(flat))(*flat)
    lab_len = (C.c_int * mb)(*[len(l) for l in labels])
    in_len = None if input_lengths is None else (C.c_int * mb)(*[int(t) for t in input_lengths])
    hyp_ld = max(1, acts.shape[0] if input_lengths is None else max(int(t) for t in input_lengths))
    errors = np.zeros(mb, np.int32)
    hyp_lens = np.zeros(mb, np.int32)
    hyps = np.zeros((mb, hyp_ld), np.int32)
    ip = C.POINTER(C.c_int)
    rc = lib.aslp_ctc_token_errors(ptr(acts), dim(acts), in_len, mb, flat_c, lab_len, errors.ctypes.data_as(ip), hyp_lens.ctypes.data_as(ip),
                                   hyps.ctypes.data_as(ip), hyp_ld)
    check_error()
    if rc != 0:
        raise ValueError("aslp_ctc_token_errors argument error %d" % rc)
    return errors, [hyps[n, :hyp_lens[n]].tolist() for n in range(mb)]


def gather_stream_rows(dst, sources, src_frame):
    """aslp_gather_stream_rows (include/aslp_kernels.h): dst [B*S x D] (a device tensor or a view with a row stride >= D); row r receives row
    src_frame[r] of sources[r % S], or +0.0 where src_frame[r] == -1.  sources: S device matrices with at least D columns (views welcome), None
    for a stream without rows.  src_frame: B*S host integers.  A plan that points outside a source raises and launches nothing."""
    import numpy as np
    from ._lib import StreamSrc
    _chk(dst)
    S = len(sources)
    rows, D = dst.shape
    if S == 0 or rows % S:
        raise ValueError("dst rows must be a multiple of the number of streams")
    plan = np.ascontiguousarray(src_frame, dtype=np.int32)
    if plan.shape != (rows,):
        raise ValueError("src_frame must hold one entry per dst row")
    table = (StreamSrc * S)()
    for s, m in enumerate(sources):
        if m is None or m.shape[0] == 0:
            table[s].base, table[s].stride, table[s].rows = None, 0, 0
            continue
        _chk(m)
        if m.dim() != 2 or m.shape[1] < D:
            raise ValueError("source %d must be a matrix of at least %d columns" % (s, D))
        table[s].base, table[s].stride, table[s].rows = m.data_ptr(), dim(m).stride, m.shape[0]
    table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dst.device)
    plan_dev = torch.from_numpy(plan).to(dst.device)
    rc = lib.aslp_gather_stream_rows(ptr(dst), dim(dst).stride, rows // S, S, D, table, ptr(table_dev), plan.ctypes.data_as(C.POINTER(C.c_int32)),
                                     ptr(plan_dev))
    check_error()
    if rc != 0:
        raise RuntimeError("aslp_gather_stream_rows refused its arguments")


def stream_batch_on_host(n):
    """1: SequenceDataReader and the chunked stream tools assemble their batches on the host; 0: gathered on the device; -1: what
    ASLP_STREAM_BATCH_HOST said.  Read when a reader is opened."""
    lib.aslp_stream_batch_on_host(int(n))


def device_to_host_syncs():
    """aslp_device_to_host_syncs (include/aslp_device.h): device-to-host copies of the engine so far, each of which waited for the stream"""
    return int(lib.aslp_device_to_host_syncs())


def ctc_errors_on_host(n):
    """1: the token errors of the CTC losses (and of ctc_token_errors) take the host loop; 0: the device kernel wherever it serves the batch;
    -1: what ASLP_CTC_ERRORS_HOST said"""
    lib.aslp_ctc_errors_on_host(int(n))


# ---- depthwise temporal filters (csrc/temporal.hip; nnet-cfsmn-component.h:170-262, nnet-row-convolution.cc:105-186) ----
def fsmn_forward(out, x, coef, past, future):
    """out[t] = x[t] + sum_j coef[j] .* x[t + j - past]; coef [(past + future + 1) x D]"""
    lib.aslp_fsmn_filter(ptr(_chk(out)), dim(out).stride, ptr(_chk(x)), dim(x).stride, ptr(_chk(coef)), dim(coef).stride, x.shape[1], past, future,
                         x.shape[0], 0)
    check_error()


def fsmn_backward(in_diff, coef_corr, coef, x, out_diff, past, future, clip=0.0, lr=0.0):
    """one launch: in_diff (reversed filter over out_diff), coef_corr (tap gradients, clipped), and with lr != 0 coef += -lr coef_corr"""
    lib.aslp_fsmn_backward(ptr(_chk(in_diff)), dim(in_diff).stride, ptr(_chk(coef_corr)), dim(coef_corr).stride, ptr(_chk(coef)), dim(coef).stride,
                           ptr(_chk(x)), dim(x).stride, ptr(_chk(out_diff)), dim(out_diff).stride, x.shape[1], past, future, x.shape[0], clip, lr)
    check_error()


def rowconv_forward(out, x, w, seq_len, K):
    """rows t * S + s; w dense [D x (K + 1)]; seq_len int32 [S] on the device"""
    S = seq_len.numel()
    lib.aslp_rowconv_forward(ptr(_chk(out)), dim(out).stride, ptr(_chk(x)), dim(x).stride, ptr(w), x.shape[1], K, x.shape[0] // S, S, ptr(seq_len))
    check_error()


def rowconv_backward(in_diff, w_diff, x, out_diff, w, seq_len, K, w_corr=None, momentum=0.0, lr=0.0):
    """in_diff and the tap gradients from one pass over x / out_diff; with w_corr given also the momentum + SGD step"""
    S = seq_len.numel()
    lib.aslp_rowconv_backward_fused(ptr(_chk(in_diff)), dim(in_diff).stride, ptr(w_diff), ptr(_chk(x)), dim(x).stride, ptr(_chk(out_diff)),
                                    dim(out_diff).stride, ptr(w), x.shape[1], K, x.shape[0] // S, S, ptr(seq_len), ptr(w_corr), momentum, lr,
                                    1 if w_corr is not None else 0)
    check_error()

