// ctc-token-errors.h -- the token errors of a CTC batch counted on the device and booked later, shared by the two losses (WarpCtc:
// warp-ctc.h, Ctc: ctc-loss.h).  Enqueue() queues argmax + the token-errors kernel + the copy of the results behind the loss on the main
// stream and returns; Settle() waits for them and books them, CountTokens(errors[s], label[s].size()) once per utterance in utterance
// order -- the order the host loop books them in, which matters because the book's error total is a float.  The losses settle before
// anything reads or adds to the book: at the top of the next Eval* and ErrorRate*, in Report() and in the token accessors.
#pragma once
#include <vector>

#include "aslp_ctc.h"
#include "ctc-cost-book.h"
#include "ctc_errors.h"
#include "cu-matrix.h"

namespace aslp {

class DeferredTokenErrors {
 public:
  // false: the host path is asked for (aslp_ctc_errors_on_host(1) / ASLP_CTC_ERRORS_HOST=1) or the batch is not served; nothing is queued
  bool Enqueue(const std::vector<int32> &frame_num_utt, const CuMatrixBase &net_out, const std::vector<std::vector<int32>> &label) {
    const int num_seq = frame_num_utt.size();
    if (ctc_errors_host_path() || num_seq == 0 || (int)label.size() < num_seq) return false;
    flat_.clear();
    ref_len_.resize(num_seq);
    for (int s = 0; s < num_seq; s++) {
      flat_.insert(flat_.end(), label[s].begin(), label[s].end());
      ref_len_[s] = label[s].size();
    }
    if (!job_.Enqueue(net_out.Data(), net_out.Dim(), frame_num_utt.data(), num_seq, flat_.data(), ref_len_.data(), false)) return false;
    ctc_errors_note_path(1);
    return true;
  }
  void Settle(CtcCostBook *book) {
    if (!job_.Pending()) return;
    if (!job_.Wait()) ASLP_ERR << "CTC token errors: the device results did not arrive";
    for (size_t s = 0; s < ref_len_.size(); s++) book->CountTokens(job_.Errors(s), ref_len_[s]);
  }

 private:
  CtcErrorsJob job_;
  std::vector<int> flat_, ref_len_;
};

}  // namespace aslp
