/*
 * aslp_ctc.h -- CTC loss C ABI of libaslp_hip.so (boundary B5 of SURVEY.md §8b).
 *
 * Drop-in for the reference's vendored Warp-CTC interface, src/warp-ctc/include/ctc.h:16-122:
 * same names, argument order, status enum and ctcComputeInfo layout, so
 * src/aslp-nnet/warp-ctc.cc:33-198 (WarpCtc::EvalGpu) links against this library unchanged.
 * Semantics follow the reference CPU implementation (cpu_ctc.h:158-428), which is the parity
 * oracle: blank = 0; softmax is applied internally; `gradients` is w.r.t. the UN-normalised
 * activations and must be zeroed by the caller (rows t >= input_lengths[n] and infeasible
 * utterances are left untouched); an utterance with L + repeats > T gets cost 0.
 *
 * Only info.loc == CTC_GPU is served (activations / gradients / workspace in device memory,
 * labels / lengths / costs in host memory, kernels on info.stream).  CTC_CPU returns
 * CTC_STATUS_EXECUTION_FAILED: this library has no CPU path.
 */
#ifndef ASLP_CTC_H_
#define ASLP_CTC_H_
#include <stddef.h>

#include "aslp_matrixdim.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct CUstream_st *CUstream; /* = hipStream_t; kept for source compatibility (ctc.h:14) */

typedef enum {
  CTC_STATUS_SUCCESS = 0,
  CTC_STATUS_MEMOPS_FAILED = 1,
  CTC_STATUS_INVALID_VALUE = 2,
  CTC_STATUS_EXECUTION_FAILED = 3,
  CTC_STATUS_UNKNOWN_ERROR = 4
} ctcStatus_t; /* ctc.h:16-22 */

const char *ctcGetStatusString(ctcStatus_t status); /* ctc.h:28 */

typedef enum { CTC_CPU = 0, CTC_GPU = 1 } ctcComputeLocation; /* ctc.h:30-33 */

struct ctcComputeInfo { /* ctc.h:40-46 */
  ctcComputeLocation loc;
  union {
    unsigned int num_threads;
    CUstream stream;
  };
};
#ifndef __cplusplus
typedef struct ctcComputeInfo ctcComputeInfo;
#endif

/* ctc.h:88-97.  activations / gradients: (t, n, p) dense, element (t*minibatch + n)*alphabet_size + p */
ctcStatus_t compute_ctc_loss(const float *const activations, float *gradients, const int *const flat_labels,
                             const int *const label_lengths, const int *const input_lengths, int alphabet_size, int minibatch,
                             float *costs, void *workspace, struct ctcComputeInfo info);

/* ctc.h:116-120 */
ctcStatus_t get_workspace_size(const int *const label_lengths, const int *const input_lengths, int alphabet_size, int minibatch,
                               struct ctcComputeInfo info, size_t *size_bytes);

int get_warpctc_version(void);

/* Extension used by the host engine's WarpCtc loss (replaces the de-stride / malloc / row copy-back
 * sequence of aslp-nnet/warp-ctc.cc:85-147): same computation on row-padded device matrices, row
 * (t*minibatch + n) at acts + (t*minibatch + n)*ld_acts; gradient rows of frames t < input_lengths[n]
 * are written, all others left untouched; workspace is library-owned; runs on the aslp_set_stream() stream. */
ctcStatus_t aslp_ctc_loss_strided(const float *acts, int ld_acts, float *grads, int ld_grads, const int *flat_labels,
                                  const int *label_lengths, const int *input_lengths, int alphabet_size, int minibatch, float *costs);


/* Eesen CTC on POST-softmax outputs (Ctc::EvalParallel, aslp-nnet/ctc-loss.cc:115-227; kernels
 * aslp-cudamatrix/cu-kernels.cu:3276-3534): diff rows of frames t < frame_num[n] receive y - posterior (the
 * unclipped value the reference forms before its loss check), others are left untouched;
 * pzx_host[n] = log p(z|x) (-1e30 = the reference's log_zero_ when there is no alignment). */
ctcStatus_t aslp_eesen_ctc_mseq(const float *net_out, int ld, float *diff, int ld_diff, const int *flat_labels, const int *label_lengths,
                                const int *frame_num, int alphabet_size, int minibatch, float *pzx_host);

/* CTC token errors on the device (WarpCtc::ErrorRate warp-ctc.cc:487-529, Ctc::ErrorRate / ErrorRateMSeq ctc-loss.cc:346-424): per
 * utterance the best path -- argmax id per frame (first strict maximum, as aslp_find_row_max_id), repeats collapsed, blanks (0) dropped --
 * and its unit-cost Levenshtein distance to the reference labels.  One workgroup per utterance; hypotheses of any length, reference
 * label sequences of up to 1024 tokens: aslp_ctc_token_errors_supported() says whether a batch with these maxima is served.  A batch
 * that is not, or every batch under aslp_ctc_errors_on_host(1) / ASLP_CTC_ERRORS_HOST=1 (read once per process; on < 0 gives the
 * decision back to the environment), takes the host path, whole: argmax launch, blocking copy of the ids, host loop.
 * aslp_ctc_errors_last_path(): which path the last call took (this one, or an ErrorRate* of the loss classes): 0 host, 1 device.
 *
 * aslp_ctc_token_errors is the synchronous form: net_out on the device, utterance s of num_seq owns rows f * num_seq + s, f < frames[s];
 * frames == NULL means one sequence of d.rows frames.  errors[s], hyp_lens[s] and (hyps != NULL) the first min(hyp_lens[s], hyp_ld)
 * tokens of hypothesis s at hyps + s * hyp_ld are written on the host.  Returns 0, 1 = bad arguments, 2 = a runtime failure
 * (aslp_get_last_error()).  Runs on the aslp_set_stream() stream. */
int aslp_ctc_token_errors_supported(int max_frames, int max_label_len);
int aslp_ctc_token_errors(const float *net_out, MatrixDim d, const int *frames, int num_seq, const int *flat_labels,
                          const int *label_lengths, int *errors, int *hyp_lens, int *hyps, int hyp_ld);
void aslp_ctc_errors_on_host(int on);
int aslp_ctc_errors_on_host_get(void);
int aslp_ctc_errors_last_path(void);

#ifdef __cplusplus
}
#endif
#endif
