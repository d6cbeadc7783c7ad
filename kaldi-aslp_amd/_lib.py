"""ctypes binding of libaslp_hip.so (the C ABI declared in include/*.h).

The library is the product: if it is missing this module raises -- there is no CPU or
PyTorch fallback for any op (oracle/ is test infrastructure and is never imported here).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libaslp_hip.so")


class MatrixDim(C.Structure):
    """cu-matrixdim.h:52-56"""
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("stride", C.c_int32)]


class Dim3(C.Structure):
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("z", C.c_uint32)]


class PlanesOut(C.Structure):
    """aslp_planes_out (include/aslp_kernels.h)"""
    _fields_ = [("hi", C.c_void_p), ("lo", C.c_void_p), ("ld", C.c_int), ("slot", C.c_void_p), ("parts", C.c_void_p), ("nparts", C.c_int), ("planes_written", C.c_int)]


class XentBlock(C.Structure):
    """aslp_xent_block (include/aslp_kernels.h)"""
    _fields_ = [("offset", C.c_int), ("cols", C.c_int), ("weight", C.c_float), ("rowstats", C.c_void_p)]


class GemmEpilogue(C.Structure):
    _fields_ = [("bias", C.c_void_p), ("clip", C.c_float), ("W", C.c_void_p), ("ldw", C.c_int),
                ("w_alpha", C.c_float), ("act_out", C.c_void_p), ("ld_act", C.c_int), ("act", C.c_int),
                ("colsum", C.c_void_p), ("colsum_beta", C.c_float), ("colsum_w", C.c_void_p), ("colsum_w_alpha", C.c_float),
                ("colstats", C.c_void_p), ("colstats_ld", C.c_int), ("c_src", C.c_void_p), ("ld_c_src", C.c_int),
                ("planes", PlanesOut), ("planes_of", C.c_int), ("wmax_parts", C.c_void_p), ("cmax_parts", C.c_void_p),
                ("bound_w_parts", C.c_void_p), ("bound_c_parts", C.c_void_p), ("bound_n", C.c_int), ("amax_parts", C.c_void_p)]


class GruSeq(C.Structure):
    """aslp_gru_seq (include/aslp_kernels.h)"""
    _fields_ = [("y", C.c_void_p), ("d", C.c_void_p), ("w_zr", C.c_void_p), ("w_m", C.c_void_p), ("ldw_zr", C.c_int), ("ldw_m", C.c_int),
                ("ld", C.c_int), ("T", C.c_int), ("S", C.c_int), ("H", C.c_int), ("s_begin", C.c_int), ("s_count", C.c_int)]


class SeqDir(C.Structure):
    """aslp_lstm_seq_dir (include/aslp_kernels.h)"""
    _fields_ = [("y", C.c_void_p), ("d", C.c_void_p), ("w", C.c_void_p), ("peep_i", C.c_void_p), ("peep_f", C.c_void_p), ("peep_o", C.c_void_p),
                ("seq_lengths", C.c_void_p), ("reverse", C.c_int), ("skip_first_product", C.c_int), ("w_first", C.c_void_p),
                ("ldw_first", C.c_int), ("k_first", C.c_int), ("col_first", C.c_int)]


class Seq(C.Structure):
    """aslp_lstm_seq (include/aslp_kernels.h)"""
    _fields_ = [("dir", SeqDir * 2), ("ndir", C.c_int), ("ld", C.c_int), ("ldw", C.c_int), ("T", C.c_int), ("S", C.c_int), ("C", C.c_int),
                ("cifg", C.c_int), ("grad_partial", C.c_void_p), ("grad_ld", C.c_int), ("s_begin", C.c_int), ("s_count", C.c_int),
                ("dmax_parts", C.c_void_p * 2)]


class StepDir(C.Structure):
    """aslp_lstm_step_dir (include/aslp_kernels.h)"""
    _fields_ = [("y_cur", C.c_void_p), ("y_prev", C.c_void_p), ("d_cur", C.c_void_p), ("d_next", C.c_void_p), ("y_next", C.c_void_p),
                ("w", C.c_void_p), ("peep_i", C.c_void_p), ("peep_f", C.c_void_p), ("peep_o", C.c_void_p), ("seq_lengths", C.c_void_p),
                ("t", C.c_int), ("has_next", C.c_int), ("no_product", C.c_int)]


class Step(C.Structure):
    """aslp_lstm_step (include/aslp_kernels.h)"""
    _fields_ = [("dir", StepDir * 2), ("ndir", C.c_int), ("ld", C.c_int), ("ldw", C.c_int), ("S", C.c_int), ("C", C.c_int), ("cifg", C.c_int)]


class StepH(C.Structure):
    """aslp_lstm_step_h (include/aslp_kernels.h)"""
    _fields_ = [("step", Step), ("w_hi", C.c_void_p * 2), ("w_lo", C.c_void_p * 2), ("w_slot", C.c_void_p * 2), ("ldp", C.c_int)]


class GruStepH(C.Structure):
    """aslp_gru_step_h (include/aslp_kernels.h)"""
    _fields_ = [("zr_hi", C.c_void_p), ("zr_lo", C.c_void_p), ("zr_slot", C.c_void_p), ("mg_hi", C.c_void_p), ("mg_lo", C.c_void_p),
                ("mg_slot", C.c_void_p), ("ldp_zr", C.c_int), ("ldp_mg", C.c_int)]


class RnnVecGrad(C.Structure):
    """aslp_rnn_vec_grad (include/aslp_kernels.h)"""
    _fields_ = [("d", C.c_void_p), ("x", C.c_void_p), ("ldx", C.c_int), ("n", C.c_int), ("corr", C.c_void_p), ("param", C.c_void_p)]


class SodSolver(C.Structure):
    """aslp_sod_solver (include/aslp_kernels.h)"""
    _fields_ = [("solver", C.c_int), ("lr", C.c_float), ("momentum", C.c_float), ("gamma", C.c_float), ("beta1", C.c_float),
                ("beta2", C.c_float), ("corr1", C.c_float), ("corr2", C.c_float)]


class StreamSrc(C.Structure):
    """aslp_stream_src (include/aslp_kernels.h)"""
    _fields_ = [("base", C.c_void_p), ("stride", C.c_int), ("rows", C.c_int)]


class CtcComputeInfo(C.Structure):
    """warp-ctc/include/ctc.h:45-60 (ctcComputeInfo: loc + union{num_threads, stream})"""
    _fields_ = [("loc", C.c_int), ("stream_or_threads", C.c_void_p)]


def _load():
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libaslp_hip.so not found at %s: build it with `make -C kaldi-aslp_amd` "
            "(or __graft_entry__.build()). There is no fallback path." % LIB_PATH)
    return C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)


lib = _load()

_vp, _f, _i, _d3, _md = C.c_void_p, C.c_float, C.c_int, Dim3, MatrixDim


def _sig(name, restype, *argtypes):
    fn = getattr(lib, name)
    fn.restype = restype
    fn.argtypes = list(argtypes)
    return fn


# runtime
_sig("aslp_set_stream", None, _vp)
_sig("aslp_get_stream", _vp)
_sig("aslp_get_last_error", _i, C.c_char_p, _i)
_sig("aslp_device_sync", _i)
_sig("aslp_version", C.c_char_p)

# elementwise (B1)
for _n in ("cudaF_set_const", "cudaF_add", "cudaF_scale", "cudaF_apply_pow", "cudaF_apply_floor", "cudaF_apply_ceiling"):
    _sig(_n, None, _d3, _d3, _vp, _f, _md)
for _n in ("cudaF_apply_log", "cudaF_apply_exp", "cudaF_apply_heaviside", "cudaF_invert_elements"):
    _sig(_n, None, _d3, _d3, _vp, _md)
_sig("cudaF_mul_elements", None, _d3, _d3, _vp, _vp, _md, _i)
_sig("cudaF_mul_cols_vec", None, _d3, _d3, _vp, _vp, _md)
_sig("cudaF_mul_rows_vec", None, _d3, _d3, _vp, _vp, _md)
_sig("cudaF_add_mat", None, _d3, _d3, _f, _vp, _vp, _md, _i, _i)
_sig("cudaF_add_vec_to_cols", None, _d3, _d3, _f, _vp, _f, _vp, _md)
_sig("cudaF_add_vec_to_rows", None, _d3, _d3, _f, _vp, _f, _vp, _md)
_sig("cudaF_add_mat_diag_vec", None, _d3, _d3, _f, _vp, _md, _vp, _i, _i, _vp, _f)
_sig("cudaF_add_mat_mat_elements", None, _d3, _d3, _vp, _vp, _vp, _md, _i, _i, _f, _f)
_sig("cudaF_add_row_sum_mat", None, _d3, _d3, _vp, _vp, _md, _i, _i, _f, _f)
_sig("cudaF_add_conv_mat_mat_elements", None, _d3, _d3, _vp, _vp, _vp, _md, _i, _i, _f, _f)
_sig("cudaF_sigmoid", None, _d3, _d3, _vp, _vp, _md, _i)
_sig("cudaF_tanh", None, _d3, _d3, _vp, _vp, _md, _i)
_sig("cudaF_diff_sigmoid", None, _d3, _d3, _vp, _vp, _vp, _md, _i, _i)
_sig("cudaF_diff_tanh", None, _d3, _d3, _vp, _vp, _vp, _md, _i, _i)
_sig("cudaF_regularize_l1", None, _d3, _d3, _vp, _vp, _f, _f, _md, _i)
# gathers
_sig("cudaF_copy_cols", None, _d3, _d3, _vp, _vp, _vp, _md, _i)
_sig("cudaF_add_cols", None, _d3, _d3, _vp, _vp, _vp, _md, _i)
_sig("cudaF_copy_rows", None, _d3, _d3, _vp, _vp, _vp, _md, _i)
_sig("cudaF_add_rows", None, _d3, _d3, _f, _vp, _vp, _vp, _md, _i)
_sig("cudaF_randomize", None, _d3, _d3, _vp, _vp, _vp, _md, _md)
_sig("cudaF_splice", None, _d3, _d3, _vp, _vp, _vp, _md, _md)
_sig("cudaF_copy", None, _d3, _d3, _vp, _vp, _vp, _md, _md)
_sig("cudaI32_set_const", None, _d3, _d3, _vp, C.c_int32, _md)
# reductions
_sig("cudaF_softmax_reduce", None, C.c_size_t, C.c_size_t, _vp, _vp, _md, _i)
_sig("cudaF_log_softmax_reduce", None, C.c_size_t, C.c_size_t, _vp, _vp, _md, _i)
_sig("cudaF_find_row_max_id", None, _d3, _d3, _vp, _vp, _vp, C.c_int32, _md)
_sig("cudaF_diff_xent", None, _d3, _d3, _vp, _vp, _vp, _md)
_sig("cudaF_add_diag_mat_mat", None, _i, _i, _f, _vp, _i, _vp, _i, _i, _i, _vp, _i, _i, _i, _f)
_sig("cudaF_add_vec_vec", None, _i, _i, _f, _vp, _vp, _vp, _f, _i)
_sig("cudaF_vec_sum", None, _i, _i, _vp, _vp, _i, _i)
_sig("aslp_add_row_sum_mat_vec", None, _f, _vp, _md, _f, _vp)
_sig("aslp_add_col_sum_mat_vec", None, _f, _vp, _md, _f, _vp)
_sig("aslp_add_row_sum_mat_vec_sgd", None, _f, _vp, _md, _f, _vp, _vp, _f)
_sig("aslp_vec_axpy2", None, _f, _vp, _vp, _vp, _vp, _i)
_sig("aslp_find_row_max_id", None, _vp, _md, _vp)
_sig("aslp_matrix_sum", None, _vp, _md, _vp)
_sig("aslp_copy_mat", None, _vp, _md, _vp, _i)
_sig("aslp_copy_mat_trans", None, _vp, _md, _vp, _i)
_sig("aslp_vec_axpy", None, _f, _vp, _vp, _i)
_sig("aslp_f2d", None, _vp, _vp, _i)
_sig("aslp_d2f", None, _vp, _vp, _i)
# gemm (B2)
_sig("aslp_sgemm", _i, _i, _i, _i, _i, _i, _f, _vp, _i, _vp, _i, _f, _vp, _i)
_sig("aslp_sgemm_ex", _i, _i, _i, _i, _i, _i, _f, _vp, _i, _vp, _i, _f, _vp, _i, C.POINTER(GemmEpilogue))
_sig("aslp_sgemm_pair_ex", _i, _i, _i, _i, _i, _i, _f, _vp, _vp, _i, _vp, _vp, _i, _f, _vp, _vp, _i, C.POINTER(GemmEpilogue), C.POINTER(GemmEpilogue))
_sig("aslp_gemm_split16", None, _i)
_sig("aslp_gemm_split16_tile", None, _i)
_sig("aslp_gemm_operand_planes", None, _i)
_sig("aslp_gemm_operand_planes_get", _i)
_sig("aslp_gemm_split16_ragged", None, _i)
_sig("aslp_gemm_split16_ragged_get", _i)
_sig("aslp_planes_new", _vp)
_sig("aslp_planes_free", None, _vp)
_sig("aslp_planes_convert", _i, _vp, _vp, _md)
_sig("aslp_planes_convert_with_parts", _i, _vp, _vp, _md, _i)
_sig("aslp_planes_reserve", None, _vp, _i, _i)
_sig("aslp_copy_mat_planes", _i, _vp, _md, _vp, _i, C.POINTER(PlanesOut))
_sig("aslp_planes_as_output", None, _vp, C.POINTER(PlanesOut))
_sig("aslp_sgemm_planes_ex", _i, _i, _i, _i, _i, _i, _f, _vp, _i, _vp, _vp, _i, _vp, _f, _vp, _i, C.POINTER(GemmEpilogue))
_sig("aslp_gemm_last_parts", _i)
_sig("aslp_params_changed", None)
_sig("aslp_keep_weight_planes", None, _i)
_sig("aslp_absmax_parts", None, _vp, _md, _vp)
_sig("aslp_weight_bound", None, _vp, _i, _vp, _i, _vp, _vp, _i, _f, _f, _f, _f, _vp)
_sig("aslp_gemm_profile", None, _i)
_sig("aslp_gemm_profile_reset", None)
_sig("aslp_gru_seq_supported", _i, C.POINTER(GruSeq), _i)
_sig("aslp_gru_seq_pieces", None, _i)
_sig("aslp_gru_seq_pieces_get", _i)
_sig("aslp_gru_seq_last_pieces", _i)
_sig("aslp_gemm_force_tile", None, _i)
_sig("aslp_gemm_last_tile", _i)
_sig("aslp_gemm_split16_plan", _i, _i, _i, _i, _i, _i, _i, C.POINTER(GemmEpilogue), C.POINTER(GemmEpilogue), _i, _i, C.POINTER(_i))
_sig("aslp_recurrent_last_path", _i, _i)   # include/aslp_nnet.h: 1 persistent, 2 one fused launch per timestep, 3 unfused
_sig("aslp_gemm_profile_get", C.c_long, _i, C.POINTER(C.c_double), C.POINTER(C.c_double))
_sig("aslp_gemm_profile_tile", _i, _i, C.c_char_p, _i)
_sig("aslp_gemm_profile_tile_flops", C.c_double, _i, _i, _i)
_sig("aslp_gemm_profile_dump", None)
_sig("aslp_lstm_seq_polls", C.c_uint, _i)
_sig("aslp_lstm_operand_pieces", None, _i)
_sig("aslp_lstm_operand_pieces_get", _i)
_sig("aslp_lstm_seq_last_pieces", _i)
_sig("aslp_lstm_seq_timing", None, _i, C.POINTER(C.c_ulonglong))
_sig("aslp_lstm_seq_supported", _i, C.POINTER(Seq), _i)
_sig("aslp_lstm_seq_first_product_supported_for", _i, _i, _i)
_sig("aslp_lstm_seq_fill", None, _vp, _i, _i, _i, _i, _i)
_sig("aslp_lstm_seq_forward", None, C.POINTER(Seq))
_sig("aslp_lstm_seq_backward", None, C.POINTER(Seq))
_sig("aslp_lstm_seq_last_dmax", _i)
_sig("aslp_lstm_split16", None, _i)
_sig("aslp_lstm_step_forward", None, C.POINTER(Step))
_sig("aslp_lstm_step_backward", None, C.POINTER(Step))
_sig("aslp_lstm_step_split16", None, _i)
_sig("aslp_lstm_step_split16_get", _i)
_sig("aslp_lstm_step_forward_h", None, C.POINTER(StepH))
_sig("aslp_lstm_step_backward_h", None, C.POINTER(StepH))
_sig("aslp_lstm_step_last_pieces", _i)
_sig("aslp_gru_step_pieces", None, _i)
_sig("aslp_gru_step_pieces_get", _i)
_sig("aslp_gru_step_last_pieces", _i)
_sig("aslp_gru_step_forward_h", None, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, C.POINTER(GruStepH))
_sig("aslp_gru_step_backward_h", None, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, C.POINTER(GruStepH))
_sig("aslp_fp16_operands", None, _i)
_sig("aslp_fp16_operands_get", _i)
_sig("aslp_region_profile", None, _i)
_sig("aslp_region_reset", None)
_sig("aslp_region_get", C.c_long, C.c_char_p, C.POINTER(C.c_double))
# fused
_sig("aslp_bn_forward", None, _vp, _md, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f)
_sig("aslp_bn_backward", None, _vp, _md, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _f, _vp, _i)
# depthwise temporal filters (csrc/temporal.hip)
_sig("aslp_fsmn_filter", None, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _i)
_sig("aslp_fsmn_backward", None, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _f, _f)
_sig("aslp_rowconv_forward", None, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _vp)
_sig("aslp_rowconv_backward_fused", None, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _f, _f, _i)
_sig("aslp_rowconv_backward", None, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _vp)
_sig("aslp_rowconv_wgrad", None, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp)
_sig("aslp_fsmn_coef_grad", None, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _f)
_sig("aslp_rowconv_path", _i, _i, _i, _i, _i, _i, _vp, _vp, _vp)
_sig("aslp_fsmn_path", _i, _i, _i, _i, _i, _i, _i)
_sig("aslp_bn_apply", None, _vp, _md, _vp, _i, _vp, _vp, _vp, _vp)
_sig("aslp_xent_eval", None, _vp, _md, _vp, _i, _vp, _vp, _vp, _i, _vp)
_sig("aslp_bn_forward_act", None, _vp, _md, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _i)
_sig("aslp_bn_forward_stats", _i, _vp, _md, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _i, _vp, _i, _i)
_sig("aslp_bn_backward_act", None, _vp, _md, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _f, _vp, _i, _vp, _i)
_sig("aslp_bn_backward_step", None, _md, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp, _i, _vp, _i, _vp, _vp)
_sig("aslp_bn_backward_step_p", None, _md, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp, _i, _vp, _i, _vp, _vp, C.POINTER(PlanesOut))
_sig("aslp_bn_panel_supported", _i, _i, _i)
_sig("aslp_bn_path", _i, _i, _i, C.POINTER(C.c_int), C.POINTER(C.c_int))
_sig("aslp_softmax_xent_supported", _i, _i)
_sig("aslp_xent_eval_p", _i, _vp, _md, _vp, _vp, _vp, _i, _vp, _i, C.POINTER(PlanesOut))
_sig("aslp_xent_eval_rows", _i, _vp, _md, _vp, _vp, _vp, _i, _vp, _i, C.POINTER(PlanesOut))
_sig("aslp_xent_sum_rowstats", None, _vp, _i, _i, _vp)
_sig("aslp_xent_sparse_supported", _i, _i, _i)
_sig("aslp_xent_sparse_eval", _i, _vp, _md, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _i)
_sig("aslp_xent_sparse_eval_rows", _i, _vp, _md, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _i)
_sig("aslp_xent_sparse", None, _i)
_sig("aslp_xent_sparse_get", _i)
_sig("aslp_mse_eval", _i, _vp, _md, _vp, _i, _vp, C.c_float, _vp, _i, _vp, C.POINTER(PlanesOut))
_sig("aslp_mse_eval_w", _i, _vp, _md, _vp, _i, _vp, C.c_float, _vp, _i, _vp, C.POINTER(PlanesOut), _vp)
_sig("aslp_mse_batch_sums", None, _vp, _i, _i, _vp)
_sig("aslp_xent_blocks_supported", _i, _i)
_sig("aslp_xent_blocks_eval", _i, _vp, _md, C.POINTER(XentBlock), _i, _vp, _vp, _vp, _i, _i, _i, _vp, _i, C.POINTER(PlanesOut))
_sig("aslp_multitask_fused", None, _i)
_sig("aslp_device_shared", None, _i)
_sig("aslp_coop_convert", None, _i)
_sig("aslp_softmax_xent_eval", None, _vp, _md, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _i)
_sig("aslp_dropout_forward", None, _vp, _i, _vp, _md, _vp, _i, _f, C.c_ulonglong)
_sig("aslp_dropout_backward", None, _vp, _i, _vp, _md, _vp, _i, _f)
_sig("aslp_apply_clamp", None, _vp, _md, _f, _f)
_sig("aslp_vec_diff", None, _vp, _vp, _vp, _i)
_sig("aslp_sod_solve", None, C.POINTER(SodSolver), _vp, _vp, _vp, _vp, _vp, _i)
_sig("aslp_rnn_vec_grads", None, C.POINTER(RnnVecGrad), _i, _i, _i, _f, _f, _f)
_sig("aslp_scatter_add", None, _vp, _md, _vp, _vp, _vp, _i)
_sig("aslp_splice_backward", None, _vp, _md, _vp, _i, _vp, _i)
_sig("aslp_diff_relu", None, _vp, _vp, _vp, _md, _i, _i)
_sig("aslp_diff_sigmoid_p", _i, _vp, _vp, _vp, _md, _i, _i, _vp, _i, C.POINTER(PlanesOut))
_sig("aslp_diff_relu_p", _i, _vp, _vp, _vp, _md, _i, _i, _vp, _i, C.POINTER(PlanesOut))
_sig("aslp_diff_tanh_p", _i, _vp, _vp, _vp, _md, _i, _i, _vp, _i, C.POINTER(PlanesOut))
_sig("aslp_max_norm_rows", None, _vp, _md, _f)
# front-end components (csrc/conv_pool.hip)
_sig("aslp_conv_gather_patches", None, _vp, _i, _vp, _md, _i, _i, _i, _i, _i)
_sig("aslp_conv_in_diff", None, _vp, _md, _vp, _i, _i, _i, _i, _i, _i)
_sig("aslp_max_pool_forward", None, _vp, _i, _vp, _md, _i, _i, _i)
_sig("aslp_max_pool_backward", None, _vp, _i, _vp, _md, _vp, _i, _vp, _i, _i, _i, _i)
_sig("aslp_length_norm_forward", None, _vp, _i, _vp, _md, _vp)
_sig("aslp_group_pnorm_backward", None, _vp, _i, _vp, _md, _vp, _i, _vp, _i, _i, _f)
_sig("aslp_group_max_backward", None, _vp, _i, _vp, _md, _vp, _i, _vp, _i, _i)
_sig("cudaF_max", None, _d3, _d3, _vp, _vp, _md, _i)
_sig("cudaF_equal_element_mask", None, _d3, _d3, _vp, _vp, _vp, _md, _i, _i)
_sig("cudaF_group_pnorm", None, _d3, _d3, _vp, _vp, _md, _i, _i, _f)
_sig("cudaF_calc_pnorm_deriv", None, _d3, _d3, _vp, _vp, _vp, _md, _i, _i, _f)
_sig("cudaF_group_max", None, _d3, _d3, _vp, _vp, _md, _i, _i)
_sig("cudaF_calc_group_max_deriv", None, _d3, _d3, _vp, _vp, _vp, _md, _i, _i)
_sig("cudaF_mul_rows_group_mat", None, _d3, _d3, _vp, _vp, _md, _i, _i)
# multi-stream batches gathered on the device (csrc/stream_batch.hip)
_sig("aslp_gather_stream_rows", _i, _vp, _i, _i, _i, _i, C.POINTER(StreamSrc), _vp, C.POINTER(C.c_int32), _vp)
_sig("aslp_gather_stream_rows_path", _i, _vp, _i, _i, _i, C.POINTER(StreamSrc))
_sig("aslp_stream_batch_on_host", None, _i)
_sig("aslp_stream_batch_on_host_get", _i)
_sig("aslp_device_to_host_syncs", C.c_longlong)


# CTC (B5, include/aslp_ctc.h)
_sig("compute_ctc_loss", _i, _vp, _vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), _i, _i, C.POINTER(C.c_float), _vp, CtcComputeInfo)
_sig("get_workspace_size", _i, C.POINTER(C.c_int), C.POINTER(C.c_int), _i, _i, CtcComputeInfo, C.POINTER(C.c_size_t))
_sig("ctcGetStatusString", C.c_char_p, _i)
_sig("get_warpctc_version", _i)
_ip = C.POINTER(C.c_int)
_sig("aslp_ctc_token_errors_supported", _i, _i, _i)
_sig("aslp_ctc_token_errors", _i, _vp, _md, _ip, _i, _ip, _ip, _ip, _ip, _ip, _i)
_sig("aslp_ctc_errors_on_host", None, _i)
_sig("aslp_ctc_errors_on_host_get", _i)
_sig("aslp_ctc_errors_last_path", _i)


def check_error():
    """Raise if any launch since the last call failed (the reference throws via KALDI_ERR)."""
    buf = C.create_string_buffer(1024)
    if lib.aslp_get_last_error(buf, 1024):
        raise RuntimeError("libaslp_hip: " + buf.value.decode())


D3 = Dim3(1, 1, 1)
