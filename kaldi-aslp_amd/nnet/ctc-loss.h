// ctc-loss.h -- the Eesen-style Ctc loss of the host engine (src/aslp-nnet/ctc-loss.{h,cc}).
// Input is the Softmax output; Eval (one sequence) / EvalParallel (padded multi-sequence batch, row =
// t*num_seq + s), ErrorRate / ErrorRateMSeq, the abnormal-loss filter (window of 100 utterances here; ctc-cost-book.h) and the
// Report() string follow the reference.  Mechanism: the lattice runs in two launches over all sequences
// (aslp_eesen_ctc_mseq) instead of 2T row kernels + the O(T*A*(2L+1)) error kernel + 6 elementwise passes.
#pragma once
#include <string>
#include <vector>

#include "ctc-cost-book.h"
#include "ctc-token-errors.h"
#include "cu-matrix.h"

namespace aslp {

#define SUM_LOSS_CHECK 0
#define AVG_LOSS_CHECK 1
#define NONE_LOSS_CHECK 2
#define CTC_GRAD_CHECK 1  // ctc-loss.h:37: the reference ships with the average-loss check compiled in

class Ctc {
 public:
  Ctc();
  void Eval(const CuMatrixBase &net_out, const std::vector<int32> &label, CuMatrix *diff);
  void EvalParallel(const std::vector<std::string> &utt, const std::vector<int32> &frame_num_utt, const CuMatrixBase &net_out,
                    std::vector<std::vector<int32>> &label, CuMatrix *diff);
  // Token errors of the best paths against the labels, counted on the device (ctc-token-errors.h).  ErrorRate hands err and hyp back, so
  // it waits for them; ErrorRateMSeq returns without waiting and whatever reads the token totals settles first.
  // aslp_ctc_errors_on_host(1) / ASLP_CTC_ERRORS_HOST=1, or a batch the kernel does not serve, takes the host loop.
  void ErrorRate(const CuMatrixBase &net_out, const std::vector<int32> &label, float *err, std::vector<int32> *hyp);
  void ErrorRateMSeq(const std::vector<int> &frame_num_utt, const CuMatrixBase &net_out, std::vector<std::vector<int>> &label);
  void SetReportStep(int32 report_step) { book_.SetReportStep(report_step); }
  std::string Report() { token_errors_.Settle(&book_); return book_.Report(); }
  float NumErrorTokens() { token_errors_.Settle(&book_); return book_.NumErrorTokens(); }
  int32 NumRefTokens() { token_errors_.Settle(&book_); return book_.NumRefTokens(); }
  // the reference's three bookkeeping variants (ctc-loss.cc:229-302, 304-329, 331-344), over the shared book
  void StatOnly(const std::vector<std::string> &, const std::vector<int32> &frame_num_utt, const std::vector<float> &pzx_host, CuMatrix *) {
    book_.AcceptAll(frame_num_utt, pzx_host);
  }
  void StatAndLossCheck(const std::vector<std::string> &utt, const std::vector<int32> &frame_num_utt, const std::vector<float> &pzx_host,
                        CuMatrix *diff) {
    book_.DropOutOfRange(utt, frame_num_utt, pzx_host, diff);
  }
  void StatAndAverageLossCheck(const std::vector<std::string> &utt, const std::vector<int32> &frame_num_utt,
                               const std::vector<float> &pzx_host, CuMatrix *diff) {
    book_.DropOutliers(utt, frame_num_utt, pzx_host, diff, /*sane_only_during_warmup=*/true);
  }
  const std::vector<float> &LastCosts() const { return last_costs_; }  // -log p(z|x) per sequence of the last call
  double Obj() const { return book_.Obj(); }
  int32 Frames() const { return book_.Frames(); }
  int32 Sequences() const { return book_.Sequences(); }

 private:
  CtcCostBook book_;   // window of 100 utterances (ctc-loss.cc: stat_period_)
  DeferredTokenErrors token_errors_;   // the last ErrorRateMSeq batch while its counts are on their way
  std::vector<float> last_costs_;
};

}  // namespace aslp
