"""Python mirror of the host engine's Nnet / Xent (include/aslp_nnet.h), keeping the reference's
method names (src/aslp-nnet/nnet-nnet.h:38-193, nnet-loss.h:66-117).  Tensors are torch CUDA
tensors; every method is a thin call into libaslp_hip.so -- no arithmetic happens in Python."""
import ctypes as C

import torch

from ._lib import lib, check_error
from .ops import ptr, dim, _chk

_vp, _i, _f = C.c_void_p, C.c_int, C.c_float
_H = C.c_void_p


def _sig(name, restype, *argtypes):
    fn = getattr(lib, name)
    fn.restype = restype
    fn.argtypes = list(argtypes)


_sig("aslp_nnet_last_error", C.c_char_p)
_sig("aslp_set_verbose", None, _i)
_sig("aslp_nnet_init_from_proto", _i, C.c_char_p, C.c_uint, C.POINTER(_H))
_sig("aslp_nnet_read", _i, C.c_char_p, C.POINTER(_H))
_sig("aslp_nnet_write", _i, _H, C.c_char_p, _i)
_sig("aslp_nnet_copy", _i, _H, C.POINTER(_H))
_sig("aslp_nnet_free", None, _H)
_sig("aslp_nnet_set_train_options", _i, _H, _f, _f, _f, _f)
for _n in ("aslp_nnet_input_dim", "aslp_nnet_output_dim", "aslp_nnet_num_components", "aslp_nnet_num_params"):
    _sig(_n, _i, _H)
_sig("aslp_nnet_component_marker", _i, _H, _i, C.c_char_p, _i)
_sig("aslp_nnet_info", _i, _H, C.c_char_p, _i)
_sig("aslp_nnet_set_link_aliasing", _i, _H, _i)
_sig("aslp_nnet_set_layer_fusion", _i, _H, _i)
_sig("aslp_nnet_set_update_overlap", _i, _H, _i)
_sig("aslp_nnet_last_fused_activations", _i, _H)
_sig("aslp_nnet_propagate", _i, _H, _vp, _i, _i, _i, _vp, _i)
_sig("aslp_nnet_feedforward", _i, _H, _vp, _i, _i, _i, _vp, _i)
_sig("aslp_nnet_backpropagate", _i, _H, _vp, _i, _i, _i, _vp, _i)
_sig("aslp_nnet_reset_lstm_streams", _i, _H, C.POINTER(C.c_int32), _i)
_sig("aslp_nnet_set_seq_lengths", _i, _H, C.POINTER(C.c_int32), _i)
_sig("aslp_nnet_set_chunk_size", _i, _H, _i)
_sig("aslp_nnet_get_params", _i, _H, C.POINTER(_f), _i)
_sig("aslp_nnet_get_gpu_params", _i, _H, C.POINTER(_vp), C.POINTER(_i), _i)
_sig("aslp_nnet_param_writers_announce", _i, _H)
_sig("aslp_nnet_get_acc_stats", _i, _H, C.POINTER(_vp), C.POINTER(_i), _i, C.POINTER(C.POINTER(C.c_double)), _i, C.POINTER(_i))
_sig("aslp_nnet_component_output", _i, _H, _i, C.POINTER(_f), _i, _i)
_sig("aslp_nnet_component_out_diff", _i, _H, _i, C.POINTER(_f), _i, _i)
_sig("aslp_xent_create", _i, C.POINTER(_H))
_sig("aslp_xent_free", None, _H)
_sig("aslp_xent_eval_batch", _i, _H, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _i)
_sig("aslp_xent_report", _i, _H, C.c_char_p, _i)
_sig("aslp_xent_get_stats", _i, _H, C.POINTER(C.c_double))
_sig("aslp_nnet_train_step_xent", _i, _H, _H, _vp, _i, _i, _i, _vp, _vp)
_sig("aslp_xent_eval_sparse_batch", _i, _H, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _i)
_sig("aslp_nnet_train_step_xent_sparse", _i, _H, _H, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp)
_sig("aslp_mse_create", _i, C.POINTER(_H))
_sig("aslp_mse_free", None, _H)
_sig("aslp_mse_eval_batch", _i, _H, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _i)
_sig("aslp_mse_report", _i, _H, C.c_char_p, _i)
_sig("aslp_mse_get_stats", _i, _H, C.POINTER(C.c_double))
_sig("aslp_nnet_train_step_mse", _i, _H, _H, _vp, _i, _i, _i, _vp, _i, _vp)
_sig("aslp_multitask_create", _i, C.c_char_p, C.POINTER(_H))
_sig("aslp_multitask_free", None, _H)
_sig("aslp_multitask_num_tasks", _i, _H)
_sig("aslp_multitask_eval_batch", _i, _H, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _i)
_sig("aslp_multitask_report", _i, _H, C.c_char_p, _i)
_sig("aslp_multitask_avg_loss", _i, _H, C.POINTER(_f))
_sig("aslp_multitask_get_stats", _i, _H, _i, C.POINTER(_i), C.POINTER(C.c_double))
_sig("aslp_nnet_train_step_multitask", _i, _H, _H, _vp, _i, _i, _i, _vp, _vp, _i, _vp)
_sig("aslp_nnet_last_loss_fold", _i, _H)
_i32p = C.POINTER(C.c_int32)
_sig("aslp_warpctc_create", _i, C.POINTER(_H))
_sig("aslp_warpctc_free", None, _H)
_sig("aslp_warpctc_eval", _i, _H, _i32p, _i, _vp, _i, _i, _i, _i32p, _i32p, _vp, _i, C.POINTER(_f))
_sig("aslp_warpctc_error_rate", _i, _H, _i32p, _i, _vp, _i, _i, _i, _i32p, _i32p)
_sig("aslp_warpctc_report", _i, _H, C.c_char_p, _i)
_sig("aslp_warpctc_get_stats", _i, _H, C.POINTER(C.c_double))
_sig("aslp_nnet_train_step_warpctc", _i, _H, _H, _vp, _i, _i, _i, _i32p, _i, _i32p, _i32p)


def _ok(rc):
    if rc != 0:
        raise RuntimeError(lib.aslp_nnet_last_error().decode())
    check_error()


def posterior_to_csr(post, num_cols, device):
    """A posterior -- per frame a list of (pdf, weight) pairs -- as the CSR tensors (row_begin int32 [frames + 1], cols int32 [nnz],
    weights float32 [nnz]) that Xent.EvalSparse and Nnet.train_step_xent_sparse take, under the rules of the engine's PosteriorToMatrix:
    a later duplicate of a pdf wins, a pdf >= num_cols is an error, a negative one is dropped, the pdfs sorted within the frame."""
    row_begin, cols, weights = [0], [], []
    for frame in post:
        last = {}
        for pdf, w in frame:
            pdf = int(pdf)
            if pdf >= num_cols:
                raise ValueError("Out-of-bound Posterior element with index %d, higher than number of columns %d" % (pdf, num_cols))
            if pdf >= 0:
                last[pdf] = float(w)
        for pdf in sorted(last):
            cols.append(pdf)
            weights.append(last[pdf])
        row_begin.append(len(cols))
    # (an empty posterior still gets one element to point at: the entry points take no null pointer)
    return (torch.tensor(row_begin, dtype=torch.int32, device=device), torch.tensor(cols or [0], dtype=torch.int32, device=device)[:len(cols) or 1],
            torch.tensor(weights or [0.0], dtype=torch.float32, device=device)[:len(cols) or 1])


def _chk_csr(rows, row_begin, cols, weights):
    _chk(row_begin, torch.int32), _chk(cols, torch.int32), _chk(weights)
    if row_begin.numel() != rows + 1:
        raise ValueError("row_begin must hold rows + 1 offsets")
    if cols.numel() != weights.numel():
        raise ValueError("cols and weights must have one length")


class Xent:
    def __init__(self):
        self.h = _H()
        _ok(lib.aslp_xent_create(C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None) and lib is not None:
            lib.aslp_xent_free(self.h)
            self.h = None

    def Eval(self, frame_weights, net_out, diff, targets=None, labels=None):
        _chk(net_out), _chk(diff), _chk(frame_weights)
        _ok(lib.aslp_xent_eval_batch(self.h, ptr(net_out), net_out.shape[0], net_out.shape[1], dim(net_out).stride,
                                     ptr(targets), dim(targets).stride if targets is not None else 0, ptr(labels),
                                     ptr(frame_weights), ptr(diff), dim(diff).stride))

    def EvalSparse(self, frame_weights, net_out, diff, row_begin, cols, weights):
        """Eval on soft targets given as CSR device tensors (posterior_to_csr): one launch, no dense target matrix, the bits of
        Eval(targets=<the dense matrix of the same entries>); net_out holds posteriors of 1 .. 8192 classes"""
        _chk(net_out), _chk(diff), _chk(frame_weights)
        _chk_csr(net_out.shape[0], row_begin, cols, weights)
        if diff.shape != net_out.shape:
            raise ValueError("net_out and diff must have one shape")
        _ok(lib.aslp_xent_eval_sparse_batch(self.h, ptr(net_out), net_out.shape[0], net_out.shape[1], dim(net_out).stride, ptr(row_begin),
                                            ptr(cols), ptr(weights), cols.numel(), ptr(frame_weights), ptr(diff), dim(diff).stride))

    def Report(self):
        buf = C.create_string_buffer(4096)
        _ok(lib.aslp_xent_report(self.h, buf, 4096))
        return buf.value.decode()

    def GetStats(self):
        st = (C.c_double * 5)()
        _ok(lib.aslp_xent_get_stats(self.h, st))
        return dict(zip(("frames", "correct", "loss", "entropy", "likelyhood"), list(st)))


class Mse:
    """Mse (nnet-loss.h:120-164): one launch per Eval, nothing read back until Report() / GetStats()"""

    def __init__(self):
        self.h = _H()
        _ok(lib.aslp_mse_create(C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None) and lib is not None:
            lib.aslp_mse_free(self.h)
            self.h = None

    def Eval(self, frame_weights, net_out, targets, diff):
        """frame_weights: a device vector [rows], or None = ones"""
        _chk(net_out), _chk(targets), _chk(diff)
        if frame_weights is not None:
            _chk(frame_weights)
        if targets.shape != net_out.shape or diff.shape != net_out.shape:
            raise ValueError("net_out, targets and diff must have one shape")
        _ok(lib.aslp_mse_eval_batch(self.h, ptr(net_out), net_out.shape[0], net_out.shape[1], dim(net_out).stride, ptr(targets),
                                    dim(targets).stride, ptr(frame_weights), ptr(diff), dim(diff).stride))

    def Report(self):
        buf = C.create_string_buffer(4096)
        _ok(lib.aslp_mse_report(self.h, buf, 4096))
        return buf.value.decode()

    def GetStats(self):
        st = (C.c_double * 3)()
        _ok(lib.aslp_mse_get_stats(self.h, st))
        return dict(zip(("frames", "loss", "num_tgt"), list(st)))


class MultiTaskLoss:
    """MultiTaskLoss (nnet-loss.h:167-218) from the reference's objective string, e.g. "multitask,xent,3000,1.0,xent,40,0.3": all xent
    tasks in one launch, an mse task in one each, nothing read back until Report() / AvgLoss() / GetStats()"""

    def __init__(self, spec):
        self.h = _H()
        _ok(lib.aslp_multitask_create(spec.encode(), C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None) and lib is not None:
            lib.aslp_multitask_free(self.h)
            self.h = None

    def NumTasks(self):
        return lib.aslp_multitask_num_tasks(self.h)

    def Eval(self, frame_weights, net_out, diff, labels=None, targets=None):
        """net_out (the network's output), diff [rows x sum of the task dims]; labels int32 [rows x number of xent tasks], relative to the
        task, < 0 = no target; targets [rows x cols], read in the mse tasks' windows; frame_weights [rows] or None = ones"""
        _chk(net_out), _chk(diff)
        if frame_weights is not None:
            _chk(frame_weights)
        if labels is not None:
            _chk(labels, torch.int32)
        if targets is not None:
            _chk(targets)
        if diff.shape != net_out.shape or (targets is not None and targets.shape != net_out.shape):
            raise ValueError("net_out, targets and diff must have one shape")
        _ok(lib.aslp_multitask_eval_batch(self.h, ptr(net_out), net_out.shape[0], net_out.shape[1], dim(net_out).stride, ptr(labels),
                                          ptr(targets), dim(targets).stride if targets is not None else 0, ptr(frame_weights), ptr(diff),
                                          dim(diff).stride))

    def Report(self):
        buf = C.create_string_buffer(8192)
        _ok(lib.aslp_multitask_report(self.h, buf, 8192))
        return buf.value.decode()

    def AvgLoss(self):
        v = _f()
        _ok(lib.aslp_multitask_avg_loss(self.h, C.byref(v)))
        return v.value

    def GetStats(self, task):
        st, kind = (C.c_double * 5)(), _i()
        _ok(lib.aslp_multitask_get_stats(self.h, task, C.byref(kind), st))
        if kind.value == 0:
            return dict(zip(("frames", "correct", "loss", "entropy", "likelyhood"), list(st)), kind="xent")
        return dict(zip(("frames", "loss", "num_tgt"), list(st)[:3]), kind="mse")


_sig("aslp_eesenctc_create", _i, C.POINTER(_H))
_sig("aslp_eesenctc_free", None, _H)
_sig("aslp_eesenctc_eval", _i, _H, _i32p, _i, _vp, _i, _i, _i, _i32p, _i32p, _vp, _i, C.POINTER(_f))
_sig("aslp_eesenctc_error_rate", _i, _H, _i32p, _i, _vp, _i, _i, _i, _i32p, _i32p)
_sig("aslp_eesenctc_report", _i, _H, C.c_char_p, _i)
_sig("aslp_eesenctc_get_stats", _i, _H, C.POINTER(C.c_double))
_sig("aslp_randomizer_mask_generate", _i, _i, _i, _i32p)
_sig("aslp_matrix_randomizer_create", _i, _i, _i, C.POINTER(_H))
_sig("aslp_matrix_randomizer_free", None, _H)
_sig("aslp_matrix_randomizer_add_data", _i, _H, _vp, _i, _i, _i)
_sig("aslp_matrix_randomizer_randomize", _i, _H, _i32p, _i)
_sig("aslp_matrix_randomizer_next", _i, _H)
_sig("aslp_matrix_randomizer_stage_begin", _i, _H)
_sig("aslp_matrix_randomizer_stage_add", _i, _H, _vp, _i, _i)
_sig("aslp_matrix_randomizer_stage_commit", _i, _H)
_sig("aslp_matrix_randomizer_stage_state", _i, _H, C.POINTER(_i))
_sig("aslp_matrix_randomizer_state", _i, _H, C.POINTER(_i))
_sig("aslp_matrix_randomizer_value", _i, _H, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i))


def randomizer_mask(size, seed=777):
    """RandomizerMask::Generate (nnet-randomizer.cc:38-44); seed < 0 keeps the current rand() state"""
    import numpy as np
    out = np.empty(size, np.int32)
    _ok(lib.aslp_randomizer_mask_generate(int(seed), int(size), out.ctypes.data_as(_i32p)))
    return out


class MatrixRandomizer:
    """aslp-nnet/nnet-randomizer.h:67-102 on device memory"""

    def __init__(self, randomizer_size=32768, minibatch_size=256):
        self.h = _H()
        _ok(lib.aslp_matrix_randomizer_create(randomizer_size, minibatch_size, C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None) and lib is not None:
            lib.aslp_matrix_randomizer_free(self.h)
            self.h = None

    def AddData(self, m):
        _chk(m)
        _ok(lib.aslp_matrix_randomizer_add_data(self.h, ptr(m), m.shape[0], m.shape[1], dim(m).stride))

    def _state(self):
        st = (_i * 3)()
        _ok(lib.aslp_matrix_randomizer_state(self.h, st))
        return st

    def IsFull(self): return bool(self._state()[0])
    def Done(self): return bool(self._state()[1])
    def NumFrames(self): return int(self._state()[2])
    def Next(self): _ok(lib.aslp_matrix_randomizer_next(self.h))

    def Randomize(self, mask):
        a = _i32arr(mask)
        _ok(lib.aslp_matrix_randomizer_randomize(self.h, a, len(mask)))

    # staged refill (include/aslp_nnet.h): host rows go up on a copy stream while the current cache is consumed
    def StageBegin(self): _ok(lib.aslp_matrix_randomizer_stage_begin(self.h))

    def StageAdd(self, host_rows):
        import numpy as np
        a = np.ascontiguousarray(host_rows, dtype=np.float32)
        _ok(lib.aslp_matrix_randomizer_stage_add(self.h, a.ctypes.data_as(_vp), a.shape[0], a.shape[1]))

    def StageCommit(self): _ok(lib.aslp_matrix_randomizer_stage_commit(self.h))

    def StageFull(self):
        st = (_i * 2)()
        _ok(lib.aslp_matrix_randomizer_stage_state(self.h, st))
        return bool(st[0])

    def Value(self):
        """copy of the current minibatch as a torch tensor (the C++ API returns a view)"""
        p, r, c, s = _vp(), _i(), _i(), _i()
        _ok(lib.aslp_matrix_randomizer_value(self.h, C.byref(p), C.byref(r), C.byref(c), C.byref(s)))
        out = torch.empty(r.value, c.value, device="cuda")
        from ._lib import MatrixDim
        lib.aslp_copy_mat(ptr(out), MatrixDim(r.value, c.value, c.value), p, s.value)
        check_error()
        return out


def _i32arr(v):
    return (C.c_int32 * max(1, len(v)))(*[int(x) for x in v])


class SequenceReaderOptions(C.Structure):
    """aslp_sequence_reader_options (include/aslp_nnet.h)"""
    _fields_ = [("batch_size", _i), ("num_stream", _i), ("drop_len", _i), ("skip_width", _i), ("targets_delay", _i), ("skip_offset", _i)]


class SequenceBatch(C.Structure):
    """aslp_sequence_batch (include/aslp_nnet.h)"""
    _fields_ = [("feat", _vp), ("rows", _i), ("cols", _i), ("stride", _i), ("labels", _vp), ("mask", _vp), ("num_labels", _i),
                ("labels_host", _i32p), ("mask_host", C.POINTER(_f)), ("new_utt_flags", _i32p), ("num_stream", _i), ("one_hot", _i), ("done", _i)]


_sig("aslp_sequence_reader_open", _i, C.c_char_p, C.c_char_p, C.POINTER(SequenceReaderOptions), _H, C.POINTER(_H))
_sig("aslp_sequence_reader_read", _i, _H, _i, C.POINTER(SequenceBatch))
_sig("aslp_sequence_reader_done", _i, _H)
_sig("aslp_sequence_reader_free", None, _H)


class SequenceReader:
    """SequenceDataReader (aslp-nnet/data-reader.h:48-100) over two Kaldi tables: num_stream utterances side by side, batch_size frames per
    read, row t * num_stream + s.  `transform` (an Nnet, optional) is applied to every utterance on the device.  The batches are gathered on
    the device unless ops.stream_batch_on_host(1) / ASLP_STREAM_BATCH_HOST=1 was in force when the reader was opened."""

    def __init__(self, feature_rspecifier, targets_rspecifier, batch_size=20, num_stream=4, targets_delay=0, skip_width=1, skip_offset=0,
                 drop_len=0, transform=None):
        self.h = _H()
        self.transform = transform   # must outlive the reader
        o = SequenceReaderOptions(int(batch_size), int(num_stream), int(drop_len), int(skip_width), int(targets_delay), int(skip_offset))
        _ok(lib.aslp_sequence_reader_open(str(feature_rspecifier).encode(), str(targets_rspecifier).encode(), C.byref(o),
                                          transform.h if transform is not None else None, C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None) and lib is not None:
            lib.aslp_sequence_reader_free(self.h)
            self.h = None

    def Done(self):
        rc = lib.aslp_sequence_reader_done(self.h)
        if rc < 0:
            raise RuntimeError(lib.aslp_nnet_last_error().decode())
        return bool(rc)

    def Read(self, num_pdf=1 << 30):
        """one batch: dict(feat=[rows x cols] float32, labels=[n] int32 (-1: the row's target is not one-hot), mask=[n] float32 -- device
        tensors, copies of the reader's buffers --, labels_host / mask_host / new_utt_flags as numpy arrays, one_hot, done)"""
        import numpy as np
        from ._lib import MatrixDim
        b = SequenceBatch()
        _ok(lib.aslp_sequence_reader_read(self.h, int(num_pdf), C.byref(b)))
        n = b.num_labels
        feat = torch.empty(b.rows, b.cols, device="cuda")
        labels = torch.empty(n, dtype=torch.int32, device="cuda")
        mask = torch.empty(n, device="cuda")
        if b.rows and b.cols:
            lib.aslp_copy_mat(ptr(feat), MatrixDim(b.rows, b.cols, b.cols), b.feat, b.stride)
        if n:   # (bit patterns: the copy kernel computes nothing)
            lib.aslp_copy_mat(ptr(labels), MatrixDim(1, n, n), b.labels, n)
            lib.aslp_copy_mat(ptr(mask), MatrixDim(1, n, n), b.mask, n)
        check_error()
        return dict(feat=feat, labels=labels, mask=mask,
                    labels_host=np.ctypeslib.as_array(b.labels_host, shape=(n,)).copy() if n else np.zeros(0, np.int32),
                    mask_host=np.ctypeslib.as_array(b.mask_host, shape=(n,)).copy() if n else np.zeros(0, np.float32),
                    new_utt_flags=np.ctypeslib.as_array(b.new_utt_flags, shape=(b.num_stream,)).copy(),
                    one_hot=bool(b.one_hot), done=bool(b.done))


def _flat(labels):
    flat = [int(x) for l in labels for x in l]
    return _i32arr(flat), _i32arr([len(l) for l in labels])


class WarpCtc:
    """aslp-nnet/warp-ctc.h:29: Eval / ErrorRate / Report on device-resident activations."""

    def __init__(self):
        self.h = _H()
        _ok(lib.aslp_warpctc_create(C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None) and lib is not None:
            lib.aslp_warpctc_free(self.h)
            self.h = None

    def Eval(self, frame_num_utt, net_out, labels, diff=None):
        """returns (diff, costs); net_out rows are t*num_utt + s, pre-softmax activations"""
        import numpy as np
        _chk(net_out)
        if diff is None:
            diff = torch.empty_like(net_out)
        n = len(frame_num_utt)
        fl, ll = _flat(labels[:n])
        costs = np.zeros(n, np.float32)
        _ok(lib.aslp_warpctc_eval(self.h, _i32arr(frame_num_utt), n, ptr(net_out), net_out.shape[0], net_out.shape[1],
                                  dim(net_out).stride, fl, ll, ptr(diff), dim(diff).stride, costs.ctypes.data_as(C.POINTER(_f))))
        return diff, costs

    def ErrorRate(self, frame_num_utt, net_out, labels):
        _chk(net_out)
        n = len(frame_num_utt)
        fl, ll = _flat(labels[:n])
        _ok(lib.aslp_warpctc_error_rate(self.h, _i32arr(frame_num_utt), n, ptr(net_out), net_out.shape[0], net_out.shape[1],
                                        dim(net_out).stride, fl, ll))

    def Report(self):
        buf = C.create_string_buffer(4096)
        _ok(lib.aslp_warpctc_report(self.h, buf, 4096))
        return buf.value.decode()

    def GetStats(self):
        st = (C.c_double * 5)()
        _ok(lib.aslp_warpctc_get_stats(self.h, st))
        return dict(zip(("obj", "frames", "sequences", "error_tokens", "ref_tokens"), list(st)))


class Ctc:
    """aslp-nnet/ctc-loss.h:39 (Eesen-style): Eval / EvalParallel / ErrorRate[MSeq] / Report on Softmax outputs."""

    def __init__(self):
        self.h = _H()
        _ok(lib.aslp_eesenctc_create(C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None) and lib is not None:
            lib.aslp_eesenctc_free(self.h)
            self.h = None

    def _eval(self, frame_num_utt, net_out, labels, diff):
        import numpy as np
        _chk(net_out)
        if diff is None:
            diff = torch.empty_like(net_out)
        n = len(labels) if frame_num_utt is None else len(frame_num_utt)
        fl, ll = _flat(labels[:n])
        costs = np.zeros(n, np.float32)
        _ok(lib.aslp_eesenctc_eval(self.h, None if frame_num_utt is None else _i32arr(frame_num_utt), n, ptr(net_out), net_out.shape[0],
                                   net_out.shape[1], dim(net_out).stride, fl, ll, ptr(diff), dim(diff).stride,
                                   costs.ctypes.data_as(C.POINTER(_f))))
        return diff, costs

    def Eval(self, net_out, label, diff=None):
        return self._eval(None, net_out, [label], diff)

    def EvalParallel(self, frame_num_utt, net_out, labels, diff=None):
        return self._eval(frame_num_utt, net_out, labels, diff)

    def ErrorRate(self, net_out, label):
        fl, ll = _flat([label])
        _ok(lib.aslp_eesenctc_error_rate(self.h, None, 1, ptr(net_out), net_out.shape[0], net_out.shape[1], dim(net_out).stride, fl, ll))

    def ErrorRateMSeq(self, frame_num_utt, net_out, labels):
        n = len(frame_num_utt)
        fl, ll = _flat(labels[:n])
        _ok(lib.aslp_eesenctc_error_rate(self.h, _i32arr(frame_num_utt), n, ptr(net_out), net_out.shape[0], net_out.shape[1],
                                         dim(net_out).stride, fl, ll))

    def Report(self):
        buf = C.create_string_buffer(4096)
        _ok(lib.aslp_eesenctc_report(self.h, buf, 4096))
        return buf.value.decode()

    def GetStats(self):
        st = (C.c_double * 5)()
        _ok(lib.aslp_eesenctc_get_stats(self.h, st))
        return dict(zip(("obj", "frames", "sequences", "error_tokens", "ref_tokens"), list(st)))


class Nnet:
    def __init__(self, handle):
        self.h = handle

    @classmethod
    def Init(cls, proto_text, seed=777):
        h = _H()
        _ok(lib.aslp_nnet_init_from_proto(proto_text.encode(), seed, C.byref(h)))
        return cls(h)

    @classmethod
    def Read(cls, path):
        h = _H()
        _ok(lib.aslp_nnet_read(str(path).encode(), C.byref(h)))
        return cls(h)

    def Copy(self):
        h = _H()
        _ok(lib.aslp_nnet_copy(self.h, C.byref(h)))
        return Nnet(h)

    def __del__(self):
        if getattr(self, "h", None) and lib is not None:
            lib.aslp_nnet_free(self.h)
            self.h = None

    def Write(self, path, binary=True):
        _ok(lib.aslp_nnet_write(self.h, str(path).encode(), int(binary)))

    def SetTrainOptions(self, learn_rate=0.008, momentum=0.0, l2_penalty=0.0, l1_penalty=0.0):
        _ok(lib.aslp_nnet_set_train_options(self.h, learn_rate, momentum, l2_penalty, l1_penalty))

    def InputDim(self): return lib.aslp_nnet_input_dim(self.h)
    def OutputDim(self): return lib.aslp_nnet_output_dim(self.h)
    def NumComponents(self): return lib.aslp_nnet_num_components(self.h)
    def NumParams(self): return lib.aslp_nnet_num_params(self.h)

    def Marker(self, c):
        buf = C.create_string_buffer(128)
        _ok(lib.aslp_nnet_component_marker(self.h, c, buf, 128))
        return buf.value.decode()

    def Info(self):
        buf = C.create_string_buffer(1 << 16)
        _ok(lib.aslp_nnet_info(self.h, buf, 1 << 16))
        return buf.value.decode()

    def SetLinkAliasing(self, on): _ok(lib.aslp_nnet_set_link_aliasing(self.h, int(on)))
    def SetLayerFusion(self, on): _ok(lib.aslp_nnet_set_layer_fusion(self.h, int(on)))
    def SetUpdateOverlap(self, on): _ok(lib.aslp_nnet_set_update_overlap(self.h, int(on)))

    def LastFusedActivations(self):
        """Tanh / ReLU components whose output the latest Propagate took from a layer product's epilogue (include/aslp_nnet.h)"""
        return lib.aslp_nnet_last_fused_activations(self.h)

    def Propagate(self, x, out=None):
        _chk(x)
        if out is None:
            out = torch.empty(x.shape[0], self.OutputDim(), device=x.device)
        _ok(lib.aslp_nnet_propagate(self.h, ptr(x), x.shape[0], x.shape[1], dim(x).stride, ptr(out), dim(out).stride))
        return out

    def Feedforward(self, x, out=None):
        _chk(x)
        if out is None:
            out = torch.empty(x.shape[0], self.OutputDim(), device=x.device)
        _ok(lib.aslp_nnet_feedforward(self.h, ptr(x), x.shape[0], x.shape[1], dim(x).stride, ptr(out), dim(out).stride))
        return out

    def Backpropagate(self, out_diff, want_in_diff=False):
        _chk(out_diff)
        in_diff = torch.empty(out_diff.shape[0], self.InputDim(), device=out_diff.device) if want_in_diff else None
        _ok(lib.aslp_nnet_backpropagate(self.h, ptr(out_diff), out_diff.shape[0], out_diff.shape[1], dim(out_diff).stride,
                                        ptr(in_diff), dim(in_diff).stride if in_diff is not None else 0))
        return in_diff

    def ResetLstmStreams(self, flags):
        a = (C.c_int32 * len(flags))(*[int(f) for f in flags])
        _ok(lib.aslp_nnet_reset_lstm_streams(self.h, a, len(flags)))

    def SetSeqLengths(self, lens):
        a = (C.c_int32 * len(lens))(*[int(f) for f in lens])
        _ok(lib.aslp_nnet_set_seq_lengths(self.h, a, len(lens)))

    def SetChunkSize(self, n): _ok(lib.aslp_nnet_set_chunk_size(self.h, int(n)))

    def GetParams(self):
        import numpy as np
        n = self.NumParams()
        buf = np.empty(n, np.float32)
        _ok(lib.aslp_nnet_get_params(self.h, buf.ctypes.data_as(C.POINTER(_f)), n))
        return buf

    def GetGpuParams(self, writers_announce=False):
        """[(device_ptr, n_floats)] in the reference's tensor order (nnet-nnet.cc:314-325).  writers_announce: the caller promises
        lib.aslp_params_changed() after every write through these pointers (include/aslp_nnet.h); without it the net stops keeping
        anything derived from its weights from step to step (always correct, a little slower)."""
        n = lib.aslp_nnet_get_gpu_params(self.h, None, None, 0)
        if n < 0:
            _ok(1)
        ptrs = (_vp * n)()
        sizes = (_i * n)()
        lib.aslp_nnet_get_gpu_params(self.h, ptrs, sizes, n)
        if writers_announce:
            _ok(lib.aslp_nnet_param_writers_announce(self.h))
        return [(ptrs[i], sizes[i]) for i in range(n)]

    def ComponentOutput(self, c, rows, cols):
        import numpy as np
        buf = np.empty((rows, cols), np.float32)
        _ok(lib.aslp_nnet_component_output(self.h, c, buf.ctypes.data_as(C.POINTER(_f)), rows, cols))
        return buf

    def ComponentOutDiff(self, c, rows, cols):
        import numpy as np
        buf = np.empty((rows, cols), np.float32)
        _ok(lib.aslp_nnet_component_out_diff(self.h, c, buf.ctypes.data_as(C.POINTER(_f)), rows, cols))
        return buf

    def TrainStepWarpCtc(self, ctc, x, frame_num_utt, labels):
        """SetSeqLengths -> Propagate -> WarpCtc::Eval + ErrorRate -> Backpropagate(+Update)."""
        _chk(x)
        n = len(frame_num_utt)
        fl, ll = _flat(labels[:n])
        _ok(lib.aslp_nnet_train_step_warpctc(self.h, ctc.h, ptr(x), x.shape[0], x.shape[1], dim(x).stride, _i32arr(frame_num_utt), n, fl, ll))

    def train_step_mse(self, mse, x, targets, frame_weights=None):
        """Propagate -> Mse::Eval -> Backpropagate(+Update), all on the device; targets [rows x OutputDim()], frame_weights [rows] or None."""
        _chk(x), _chk(targets)
        if frame_weights is not None:
            _chk(frame_weights)
        if targets.shape[0] != x.shape[0] or targets.shape[1] != self.OutputDim():
            raise ValueError("targets must be [rows x OutputDim()]")
        _ok(lib.aslp_nnet_train_step_mse(self.h, mse.h, ptr(x), x.shape[0], x.shape[1], dim(x).stride, ptr(targets), dim(targets).stride,
                                         ptr(frame_weights)))

    def train_step_multitask(self, loss, x, labels=None, targets=None, frame_weights=None):
        """Propagate -> MultiTaskLoss -> Backpropagate(+Update), all on the device; labels int32 [rows x number of xent tasks], targets
        [rows x OutputDim()] (mse tasks), frame_weights [rows] or None.  A final <BlockSoftmax> whose blocks are the (all xent) tasks is
        left to the loss kernel: LastLossFold() == 2."""
        _chk(x)
        for t, dt in ((labels, torch.int32), (targets, torch.float32), (frame_weights, torch.float32)):
            if t is not None:
                _chk(t, dt)
        if labels is not None and labels.shape[0] != x.shape[0]:
            raise ValueError("labels must be [rows x number of xent tasks]")
        if targets is not None and (targets.shape[0] != x.shape[0] or targets.shape[1] != self.OutputDim()):
            raise ValueError("targets must be [rows x OutputDim()]")
        _ok(lib.aslp_nnet_train_step_multitask(self.h, loss.h, ptr(x), x.shape[0], x.shape[1], dim(x).stride, ptr(labels), ptr(targets),
                                               dim(targets).stride if targets is not None else 0, ptr(frame_weights)))

    def train_step_xent_sparse(self, xent, x, row_begin, cols, weights, frame_weights=None):
        """Propagate -> Xent::EvalSparse -> Backpropagate(+Update), all on the device, on soft targets given as CSR device tensors
        (posterior_to_csr); frame_weights [rows] or None.  A final Softmax of 513 .. 8192 classes is left to the loss kernel."""
        _chk(x)
        _chk_csr(x.shape[0], row_begin, cols, weights)
        if frame_weights is not None:
            _chk(frame_weights)
        _ok(lib.aslp_nnet_train_step_xent_sparse(self.h, xent.h, ptr(x), x.shape[0], x.shape[1], dim(x).stride, ptr(row_begin), ptr(cols),
                                                 ptr(weights), cols.numel(), ptr(frame_weights)))

    def LastLossFold(self):
        """what the latest train step left to its loss kernel: 0 nothing, 1 the final Softmax, 2 the final BlockSoftmax"""
        return lib.aslp_nnet_last_loss_fold(self.h)

    def TrainStepXent(self, xent, x, labels, frame_weights=None):
        """Propagate -> Xent::Eval -> Backpropagate(+Update), all on the device."""
        _chk(x), _chk(labels, torch.int32)
        _ok(lib.aslp_nnet_train_step_xent(self.h, xent.h, ptr(x), x.shape[0], x.shape[1], dim(x).stride, ptr(labels), ptr(frame_weights)))
