// ctc_errors.h -- CTC token errors on the device (ctc_errors.hip): best path + edit distance of a batch behind the row argmax.
#pragma once
#include "aslp_matrixdim.h"

namespace aslp {

// does the switch (aslp_ctc_errors_on_host / ASLP_CTC_ERRORS_HOST=1) ask for the host path?
bool ctc_errors_host_path();
// what aslp_ctc_errors_last_path() answers: every ErrorRate* / aslp_ctc_token_errors call says which path it took (0 host, 1 device)
void ctc_errors_note_path(int device);

// One batch in flight: argmax + the token-errors kernel + the copy of the results into page-locked memory, all on the calling thread's
// current stream, behind one event.  Enqueue() returns without waiting; Wait() blocks until the results are readable.  The page-locked
// staging and result blocks and the scratch slot are grow-only: a steady loop allocates nothing.  The staging is rewritten by the next
// Enqueue() only, which first waits for the batch before it -- and with it for the upload that read the staging.
class CtcErrorsJob {
 public:
  CtcErrorsJob() = default;
  ~CtcErrorsJob();
  CtcErrorsJob(const CtcErrorsJob &) = delete;
  CtcErrorsJob &operator=(const CtcErrorsJob &) = delete;
  // frames == NULL: one sequence of d.rows frames.  false = the batch is not served (or a runtime call failed, error set): nothing is
  // pending and the caller takes the host path.  want_hyps: the hypotheses come back too (Hyp()).
  bool Enqueue(const float *net_out, MatrixDim d, const int *frames, int num_seq, const int *flat_labels, const int *label_lengths,
               bool want_hyps);
  bool Pending() const { return pending_; }
  bool Wait();   // false = nothing was pending, or the wait failed (error set)
  // results of the batch last waited for
  int Errors(int s) const { return h_res_[2 * s]; }
  int HypLen(int s) const { return h_res_[2 * s + 1]; }
  const int *Hyp(int s) const { return h_res_ + 2 * num_seq_ + (long)s * hyp_ld_; }   // want_hyps only

 private:
  bool Reserve(int **blk, long *cap, long ints);
  int *h_stage_ = nullptr, *h_res_ = nullptr;   // page-locked
  long stage_cap_ = 0, res_cap_ = 0;            // in ints
  void *done_ = nullptr;                        // hipEvent_t
  int num_seq_ = 0, hyp_ld_ = 0;
  bool pending_ = false;
};

}  // namespace aslp
