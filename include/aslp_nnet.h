/*
 * aslp_nnet.h -- C handle API over the host engine's Nnet / loss objects (boundary B4 of
 * SURVEY.md §8b), so that non-C++ hosts (tests, bench.py, other runtimes) can drive the same
 * objects a C++ caller links directly (kaldi-aslp_amd/nnet/nnet-nnet.h).
 *
 * Each function mirrors one method of the reference's kaldi::aslp_nnet::Nnet
 * (src/aslp-nnet/nnet-nnet.h:38-193) or loss class (nnet-loss.h:35-218); the reference line is
 * cited per function.  Reference methods throw (KALDI_ERR); here every function returns 0 on
 * success and non-zero on error, with the message available from aslp_nnet_last_error().
 * Matrices are DEVICE pointers, row-major fp32, with an explicit stride in elements.
 */
#ifndef ASLP_NNET_H_
#define ASLP_NNET_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct aslp_nnet_s *aslp_nnet_t;
typedef struct aslp_xent_s *aslp_xent_t;
typedef struct aslp_mse_s *aslp_mse_t;

const char *aslp_nnet_last_error(void);
void aslp_set_verbose(int level);

/* Nnet::Init (nnet-nnet.cc:570-612) from <NnetProto> text; srand(seed) first like aslp-nnet-init. */
int aslp_nnet_init_from_proto(const char *proto_text, unsigned seed, aslp_nnet_t *out);
int aslp_nnet_read(const char *path, aslp_nnet_t *out);                 /* Nnet::Read  :615 */
int aslp_nnet_write(aslp_nnet_t n, const char *path, int binary);       /* Nnet::Write :648 */
int aslp_nnet_copy(aslp_nnet_t n, aslp_nnet_t *out);                    /* copy ctor   :41  */
void aslp_nnet_free(aslp_nnet_t n);

int aslp_nnet_set_train_options(aslp_nnet_t n, float learn_rate, float momentum, float l2_penalty, float l1_penalty); /* :834 */
int aslp_nnet_input_dim(aslp_nnet_t n);
int aslp_nnet_output_dim(aslp_nnet_t n);
int aslp_nnet_num_components(aslp_nnet_t n);
int aslp_nnet_num_params(aslp_nnet_t n);
int aslp_nnet_component_marker(aslp_nnet_t n, int c, char *buf, int buflen);
int aslp_nnet_info(aslp_nnet_t n, char *buf, int buflen);               /* Nnet::Info :714 */
int aslp_nnet_set_link_aliasing(aslp_nnet_t n, int on);                 /* engine switch, see nnet-nnet.h */
int aslp_nnet_set_layer_fusion(aslp_nnet_t n, int on);                  /* engine switch: BatchNormalization + Sigmoid in one kernel pair */
int aslp_nnet_set_update_overlap(aslp_nnet_t n, int on);                /* engine switch: AffineTransform::Update on a side stream */

/* out: [rows x OutputDim].  Nnet::Propagate :191 / Feedforward :218 */
int aslp_nnet_propagate(aslp_nnet_t n, const float *in, int rows, int cols, int stride, float *out, int out_stride);
int aslp_nnet_feedforward(aslp_nnet_t n, const float *in, int rows, int cols, int stride, float *out, int out_stride);
/* in_diff may be NULL.  Nnet::Backpropagate :206 (Update of every updatable component included) */
int aslp_nnet_backpropagate(aslp_nnet_t n, const float *out_diff, int rows, int cols, int stride, float *in_diff, int in_diff_stride);

int aslp_nnet_reset_lstm_streams(aslp_nnet_t n, const int32_t *flags_host, int num_streams);   /* :473 */
int aslp_nnet_set_seq_lengths(aslp_nnet_t n, const int32_t *lengths_host, int num_streams);    /* :498 */
int aslp_nnet_set_chunk_size(aslp_nnet_t n, int chunk_size);                                   /* :532 */
/* Which kernels carried the recurrence of the calling thread's latest recurrent component pass (LSTM family, GruStreams): backward == 0
 * the latest Propagate, != 0 the latest Backpropagate.  Read-only, like aslp_gemm_last_tile: tests assert it so that a case meant for one
 * path cannot move to another unnoticed.  In a net of several recurrent components it speaks of the one that ran last. */
enum {
  ASLP_RECURRENT_NONE = 0,        /* no recurrent pass on this thread yet */
  ASLP_RECURRENT_PERSISTENT = 1,  /* one launch for all timesteps (csrc/rnn_persistent.hip) */
  ASLP_RECURRENT_STEP_FUSED = 2,  /* one fused launch per timestep (csrc/rnn_fused.hip, gru_fused.hip) */
  ASLP_RECURRENT_UNFUSED = 3      /* a product and cell kernels per timestep (csrc/rnn_cells.hip) */
};
int aslp_recurrent_last_path(int backward);
/* How many Tanh / ReLU components took their output from the epilogue of the layer product in front of them in n's latest Propagate
 * (Sigmoid layers, which have always done so, are not counted).  0 under aslp_nnet_set_layer_fusion(n, 0) and under the A/B switch
 * ASLP_FUSE_TANH_RELU=0 (read once per process), which sends these two activations through their own launches.  For tests. */
int aslp_nnet_last_fused_activations(aslp_nnet_t n);

/* Nnet::GetParams (:296) -> host buffer of NumParams floats */
int aslp_nnet_get_params(aslp_nnet_t n, float *host_buf, int buf_len);
/* Nnet::GetGpuParams (:314): device pointers + float counts (rows*stride) of every tensor, in the
 * reference's order.  Returns the number of tensors (also when max_n is too small). */
int aslp_nnet_get_gpu_params(aslp_nnet_t n, float **ptrs, int *sizes, int max_n);
/* Whoever writes through those pointers promises to call aslp_params_changed() (include/aslp_kernels.h) after every write; without this
 * promise a net whose pointers were handed out re-derives everything it keeps of its weights in every step (correct, slower).  The native
 * sync workers make the promise themselves (aslp_worker_init_param_nnet). */
int aslp_nnet_param_writers_announce(aslp_nnet_t n);
/* Nnet::GetAccStats (:327): BatchNorm running statistics. counts_host[i] = num_acc_frames of BN i. */
int aslp_nnet_get_acc_stats(aslp_nnet_t n, double **dev_ptrs, int *sizes, int max_n, double **counts_host, int max_bn, int *num_bn);
/* copy component c's forward output / output-diff buffer to the host (reference: PropagateBuffer()) */
int aslp_nnet_component_output(aslp_nnet_t n, int c, float *host_dst, int rows, int cols);
int aslp_nnet_component_out_diff(aslp_nnet_t n, int c, float *host_dst, int rows, int cols);

/* ---- Xent (nnet-loss.h:66-117) ------------------------------------------------------------ */
int aslp_xent_create(aslp_xent_t *out);
void aslp_xent_free(aslp_xent_t x);
/* dense targets [rows x cols] or (targets == NULL) one int32 label per row; frame_weights [rows]; all device */
int aslp_xent_eval_batch(aslp_xent_t x, const float *net_out, int rows, int cols, int stride, const float *targets, int tgt_stride,
                   const int32_t *labels, const float *frame_weights, float *diff, int diff_stride);
int aslp_xent_report(aslp_xent_t x, char *buf, int buflen);   /* Xent::Report nnet-loss.cc:175 */
int aslp_xent_get_stats(aslp_xent_t x, double stats[5]);      /* frames, correct, loss, entropy, likelyhood */

/* One whole training step with nothing on the host: Propagate -> Xent::Eval (labels) -> Backpropagate
 * (nnet-nnet.cc:70-154 + nnet-loss.cc:63; the loop body of aslp-nnet-train-frame.cc:109-131). */
int aslp_nnet_train_step_xent(aslp_nnet_t n, aslp_xent_t x, const float *in, int rows, int cols, int stride,
                              const int32_t *labels, const float *frame_weights);
/* Soft targets (weighted pdfs per frame: pruned teacher posteriors, smoothed alignments, lattice posteriors) as CSR in device memory:
 * row_begin [rows + 1] (row_begin[0] == 0, non-decreasing), tgt_col [nnz] (strictly increasing within a row; one outside [0, cols) is
 * skipped), tgt_w [nnz].  One launch over rows of 1 .. 8192 classes, no dense target matrix, nothing read back before report / get_stats;
 * the bits of aslp_xent_eval_batch on the dense matrix of the same entries.  net_out holds posteriors; frame_weights [rows]; all device. */
int aslp_xent_eval_sparse_batch(aslp_xent_t x, const float *net_out, int rows, int cols, int stride, const int32_t *row_begin,
                                const int32_t *tgt_col, const float *tgt_w, int nnz, const float *frame_weights, float *diff, int diff_stride);
/* aslp_nnet_train_step_xent on such targets: Propagate -> Xent::EvalSparse (in front of a final Softmax where the network leaves it to the
 * loss) -> Backpropagate.  frame_weights NULL = ones. */
int aslp_nnet_train_step_xent_sparse(aslp_nnet_t n, aslp_xent_t x, const float *in, int rows, int cols, int stride, const int32_t *row_begin,
                                     const int32_t *tgt_col, const float *tgt_w, int nnz, const float *frame_weights);
/* A/B switch (ASLP_XENT_SPARSE=0, read once per process): off = Xent::Eval on a Posterior that is not one-hot builds the dense target matrix
 * (PosteriorToMatrix) and runs the dense kernel, as before.  The two entry points above are not switched. */
void aslp_xent_sparse(int on);
int aslp_xent_sparse_get(void);

/* ---- Mse (nnet-loss.h:120-164) -------------------------------------------------------------- */
int aslp_mse_create(aslp_mse_t *out);
void aslp_mse_free(aslp_mse_t m);
/* net_out, targets [rows x cols], frame_weights [rows] (NULL = ones), diff [rows x cols]: all device.  One launch, nothing read back:
 * the loss and the frame count (int32 of the weights' sum, per minibatch) reach the host with aslp_mse_report / aslp_mse_get_stats, and
 * so does the error of a loss that is not finite. */
int aslp_mse_eval_batch(aslp_mse_t m, const float *net_out, int rows, int cols, int stride, const float *targets, int tgt_stride,
                        const float *frame_weights, float *diff, int diff_stride);
int aslp_mse_report(aslp_mse_t m, char *buf, int buflen);   /* Mse::Report nnet-loss.cc:277 */
int aslp_mse_get_stats(aslp_mse_t m, double stats[3]);      /* frames, loss, num_tgt */
/* One whole training step with nothing on the host: Propagate -> Mse::Eval -> Backpropagate (the loop body of aslp-nnet-train-mse.cc).
 * Mse reads the network's output: a final Softmax is never folded away. */
int aslp_nnet_train_step_mse(aslp_nnet_t n, aslp_mse_t m, const float *in, int rows, int cols, int stride, const float *targets,
                             int tgt_stride, const float *frame_weights);

/* ---- MultiTaskLoss (nnet-loss.h:167-218) ----------------------------------------------------- */
typedef struct aslp_multitask_s *aslp_multitask_t;
/* spec: the reference's objective string, "multitask,<xent|mse>,<dim>,<weight>[,...]"; a malformed one is an error */
int aslp_multitask_create(const char *spec, aslp_multitask_t *out);
void aslp_multitask_free(aslp_multitask_t m);
int aslp_multitask_num_tasks(aslp_multitask_t m);   /* -1: no handle */
/* net_out, diff [rows x cols], cols = the sum of the task dims: all device.  labels [rows x number of xent tasks], row-major, in task
 * order, relative to the task's first column, < 0 = no target (NULL only without an xent task).  targets: [rows x cols], read in the mse
 * tasks' windows only (NULL only without an mse task).  frame_weights [rows], NULL = ones.  net_out holds the network's output (posteriors
 * in the xent tasks' windows).  All xent tasks in one launch, an mse task in one each; nothing is read back before report / get_stats. */
int aslp_multitask_eval_batch(aslp_multitask_t m, const float *net_out, int rows, int cols, int stride, const int32_t *labels,
                              const float *targets, int tgt_stride, const float *frame_weights, float *diff, int diff_stride);
int aslp_multitask_report(aslp_multitask_t m, char *buf, int buflen);   /* MultiTaskLoss::Report nnet-loss.cc:370 */
int aslp_multitask_avg_loss(aslp_multitask_t m, float *avg_loss);
/* kind: 0 xent, stats = frames, correct, loss, entropy, likelyhood; 1 mse, stats = frames, loss, num_tgt, 0, 0 */
int aslp_multitask_get_stats(aslp_multitask_t m, int task, int *kind, double stats[5]);
/* One whole training step with nothing on the host: Propagate -> MultiTaskLoss -> Backpropagate.  Where the network ends in a
 * <BlockSoftmax> whose block dims are the task dims and every task is xent, the component is left to the loss kernel, which forms the
 * posteriors and applies the component's backward mask (aslp_nnet_last_loss_fold tells). */
int aslp_nnet_train_step_multitask(aslp_nnet_t n, aslp_multitask_t m, const float *in, int rows, int cols, int stride, const int32_t *labels,
                                   const float *targets, int tgt_stride, const float *frame_weights);
/* what the latest train step left to its loss kernel: 0 nothing, 1 the final Softmax, 2 the final BlockSoftmax */
int aslp_nnet_last_loss_fold(aslp_nnet_t n);
/* A/B switch (ASLP_MULTITASK_FUSED=0): off = the new entry points run the op sequence of MultiTaskLoss::Eval -- no fold, a dense target
 * matrix from the labels, per task Eval, Scale, copy, the component's own backward */
void aslp_multitask_fused(int on);

/* ---- WarpCtc (aslp-nnet/warp-ctc.h:29-113) -------------------------------------------------- */
typedef struct aslp_warpctc_s *aslp_warpctc_t;
int aslp_warpctc_create(aslp_warpctc_t *out);
void aslp_warpctc_free(aslp_warpctc_t w);
/* WarpCtc::Eval (warp-ctc.cc:33): net_out = pre-softmax activations [max_T*num_utt x alphabet] on the device,
 * row = t*num_utt + s; labels flat on the host with label_lengths[num_utt]; diff (device, same shape) receives the
 * filtered, +-1-clipped gradient; costs_host[num_utt] (may be NULL) the per-utterance -log p(l|x). */
int aslp_warpctc_eval(aslp_warpctc_t w, const int32_t *frame_num_utt, int num_utt, const float *net_out, int rows, int cols, int stride,
                      const int32_t *flat_labels, const int32_t *label_lengths, float *diff, int diff_stride, float *costs_host);
/* WarpCtc::ErrorRate (warp-ctc.cc:487): best-path token errors vs the labels, accumulated into the report.  Counted on the device
 * (aslp_ctc.h: aslp_ctc_token_errors*): the call queues the work on the launch stream and returns; net_out is read there, in stream
 * order, so whatever overwrites or frees it must be ordered behind this call on that stream (as everything of this library is);
 * report / get_stats / the next eval book the counts first.  The same holds for aslp_eesenctc_error_rate with frame_num_utt. */
int aslp_warpctc_error_rate(aslp_warpctc_t w, const int32_t *frame_num_utt, int num_utt, const float *net_out, int rows, int cols, int stride,
                            const int32_t *flat_labels, const int32_t *label_lengths);
int aslp_warpctc_report(aslp_warpctc_t w, char *buf, int buflen);   /* WarpCtc::Report warp-ctc.cc:531 */
/* stats = {obj, frames, sequences, error_tokens, ref_tokens} */
int aslp_warpctc_get_stats(aslp_warpctc_t w, double stats[5]);
/* Propagate -> WarpCtc::Eval -> Backpropagate (the loop body of aslp-nnet-train-warp-ctc-streams.cc) */
int aslp_nnet_train_step_warpctc(aslp_nnet_t n, aslp_warpctc_t w, const float *in, int rows, int cols, int stride,
                                 const int32_t *frame_num_utt, int num_utt, const int32_t *flat_labels, const int32_t *label_lengths);

/* ---- Ctc (Eesen-style, aslp-nnet/ctc-loss.h:39-124): input is the Softmax output ------------------------ */
typedef struct aslp_eesenctc_s *aslp_eesenctc_t;
int aslp_eesenctc_create(aslp_eesenctc_t *out);
void aslp_eesenctc_free(aslp_eesenctc_t c);
/* Ctc::EvalParallel (ctc-loss.cc:115); num_utt == 1 with frame_num_utt == NULL selects Ctc::Eval (:31) */
int aslp_eesenctc_eval(aslp_eesenctc_t c, const int32_t *frame_num_utt, int num_utt, const float *net_out, int rows, int cols, int stride,
                       const int32_t *flat_labels, const int32_t *label_lengths, float *diff, int diff_stride, float *costs_host);
int aslp_eesenctc_error_rate(aslp_eesenctc_t c, const int32_t *frame_num_utt, int num_utt, const float *net_out, int rows, int cols, int stride,
                             const int32_t *flat_labels, const int32_t *label_lengths);
int aslp_eesenctc_report(aslp_eesenctc_t c, char *buf, int buflen);
int aslp_eesenctc_get_stats(aslp_eesenctc_t c, double stats[5]);   /* obj, frames, sequences, error_tokens, ref_tokens */

/* ---- frame shuffling cache (aslp-nnet/nnet-randomizer.h:53-102) --------------------------------- */
typedef struct aslp_matrix_randomizer_s *aslp_matrix_randomizer_t;
/* RandomizerMask::Init + Generate: srand(seed) when seed >= 0, then a permutation of [0, size) in the order
 * std::random_shuffle produces with the C library generator (nnet-randomizer.cc:33-44) */
int aslp_randomizer_mask_generate(int seed, int size, int32_t *mask_host);
int aslp_matrix_randomizer_create(int randomizer_size, int minibatch_size, aslp_matrix_randomizer_t *out);
void aslp_matrix_randomizer_free(aslp_matrix_randomizer_t r);
int aslp_matrix_randomizer_add_data(aslp_matrix_randomizer_t r, const float *dev, int rows, int cols, int stride);
/* Staged refill (this library's addition, no reference counterpart): the rows of the NEXT cache go up on a copy stream while
 * the minibatches of the current one are consumed.  stage_begin() any time after randomize(); stage_add() takes host rows
 * (copied to page-locked memory, sent asynchronously); stage_commit() once the current cache is Done(): the state afterwards is
 * the one add_data() calls with the same rows would have produced (left-over rows first, data_begin 0).
 * stage_state: [0] the staged cache is full (IsFull of nnet-randomizer.h:83), [1] frames staged including the left-over rows */
int aslp_matrix_randomizer_stage_begin(aslp_matrix_randomizer_t r);
int aslp_matrix_randomizer_stage_add(aslp_matrix_randomizer_t r, const float *host, int rows, int cols);
int aslp_matrix_randomizer_stage_commit(aslp_matrix_randomizer_t r);
int aslp_matrix_randomizer_stage_state(aslp_matrix_randomizer_t r, int state[2]);
int aslp_matrix_randomizer_randomize(aslp_matrix_randomizer_t r, const int32_t *mask_host, int n);
int aslp_matrix_randomizer_next(aslp_matrix_randomizer_t r);
/* state[0..2] = IsFull, Done, NumFrames */
int aslp_matrix_randomizer_state(aslp_matrix_randomizer_t r, int state[3]);
/* Value(): a view of the current minibatch rows inside the cache (valid until the next AddData / Randomize) */
int aslp_matrix_randomizer_value(aslp_matrix_randomizer_t r, const float **dev, int *rows, int *cols, int *stride);

/* ---- SequenceDataReader (aslp-nnet/data-reader.h:48-100, data-reader.cc:178-340) ----------------------------------
 * num_stream utterances advance in parallel, batch_size frames per read, batch row t * num_stream + s; the features run targets_delay
 * frames ahead of the targets (the last frame repeats); an exhausted stream repeats its last frame and target under mask 0 and takes the
 * next utterance at the next read; with skip_width > 1 a stream trains on the frames skip_offset, skip_offset + skip_width, ... of its
 * utterance.  `transform` (may be NULL) is applied to every utterance on the device and must outlive the reader.
 * By default the batch is gathered on the device from utterances that stay there (aslp_gather_stream_rows, include/aslp_kernels.h) and no
 * read waits for the device; under aslp_stream_batch_on_host(1) / ASLP_STREAM_BATCH_HOST=1 (as it stood when the reader was opened) it is
 * assembled on the host.  Same batches either way, bit for bit. */
typedef struct aslp_sequence_reader_s *aslp_sequence_reader_t;
typedef struct {
  int batch_size, num_stream, drop_len, skip_width, targets_delay, skip_offset;
} aslp_sequence_reader_options;
typedef struct {
  const float *feat;             /* device [rows x cols], row stride `stride`; as it was when every stream was exhausted before the read */
  int rows, cols, stride;
  const int32_t *labels;         /* device [num_labels]: the row's pdf where its target is one-hot (one pair, weight 1), -1 elsewhere */
  const float *mask;             /* device [num_labels]: 1 where the row counts in the loss */
  int num_labels;                /* batch_size * num_stream */
  const int32_t *labels_host;    /* the same two on the host */
  const float *mask_host;
  const int32_t *new_utt_flags;  /* host [num_stream]: 1 where the stream took a new utterance for this batch */
  int num_stream;
  int one_hot;                   /* no label is -1: labels + mask can go to aslp_xent_eval_batch as they are */
  int done;                      /* aslp_sequence_reader_done() after this read */
} aslp_sequence_batch;
int aslp_sequence_reader_open(const char *feature_rspecifier, const char *targets_rspecifier, const aslp_sequence_reader_options *opts,
                              aslp_nnet_t transform, aslp_sequence_reader_t *out);
/* SequenceDataReader::ReadData.  num_pdf: a label >= num_pdf is an error.  The pointers in *out stay valid until the next call on r. */
int aslp_sequence_reader_read(aslp_sequence_reader_t r, int num_pdf, aslp_sequence_batch *out);
int aslp_sequence_reader_done(aslp_sequence_reader_t r);   /* 1 / 0; < 0 on error */
void aslp_sequence_reader_free(aslp_sequence_reader_t r);

#ifdef __cplusplus
}
#endif
#endif
