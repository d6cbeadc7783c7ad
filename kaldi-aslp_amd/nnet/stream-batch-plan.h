// stream-batch-plan.h -- which frame of which stream goes into which row of a multi-stream batch: the index arithmetic of
// SequenceDataReader::FillBatchBuff and of the latency-controlled chunk tools, as a plan of integers that a gather on the device
// (StreamBatcher, stream-batcher.h) or a loop on the host can carry out.  Host-only, no device types: tools/stream_plan_check.cpp
// runs it under the sanitizers.
#pragma once
#include <vector>

#include "base.h"

namespace aslp {

// Row t * S + s of a batch of B frames of S streams.
struct StreamBatchPlan {
  std::vector<int32> src_frame;    // row of stream s's source matrix that the batch row receives; -1: a row of zeros
  std::vector<int32> tgt_index;    // index into stream s's targets; -1: the stream has none (it never received an utterance)
  std::vector<BaseFloat> mask;     // 1: the row counts in the loss
  bool all_done = false;           // every stream was exhausted before the batch: nothing was planned, the cursors did not move
  void Reset(size_t rows) {
    src_frame.assign(rows, -1);
    tgt_index.assign(rows, -1);
    mask.assign(rows, 0.0f);
    all_done = false;
  }
};

inline bool AllStreamsDone(const std::vector<int32> &curt, const std::vector<int32> &lent) {
  for (size_t s = 0; s < curt.size(); s++)
    if (curt[s] < lent[s]) return false;
  return true;
}

// SequenceDataReader (data-reader.cc:272-325).  lent[s] counts the frames the stream trains on: with skip_width > 1 those are the frames
// skip_offset, skip_offset + skip_width, ... of its utterance, and target i belongs to frame i * skip_width + skip_offset.  The features are
// delayed against the targets by `delay` frames and the last frame repeats; an exhausted stream repeats its last frame and target under a
// zero mask; a stream that never received an utterance has zero rows and no target.  Advances every cursor by B.
inline void PlanSequenceBatch(int32 B, int32 delay, int32 skip_width, int32 skip_offset, std::vector<int32> *curt, const std::vector<int32> &lent,
                              StreamBatchPlan *plan) {
  const int32 S = (int32)lent.size();
  ASLP_ASSERT((int32)curt->size() == S && B >= 0 && delay >= 0 && skip_offset >= 0);
  plan->Reset((size_t)B * S);
  if (AllStreamsDone(*curt, lent)) { plan->all_done = true; return; }
  const int32 step = skip_width > 1 ? skip_width : 1, first = skip_width > 1 ? skip_offset : 0;
  for (int32 t = 0; t < B; t++) {
    for (int32 s = 0; s < S; s++) {
      const size_t row = (size_t)t * S + s;
      int32 &cur = (*curt)[s];
      if (lent[s] == 0) { cur++; continue; }
      if (cur < lent[s]) { plan->mask[row] = 1.0f; plan->tgt_index[row] = cur; }
      else plan->tgt_index[row] = lent[s] - 1;
      const int32 src = cur < lent[s] - delay ? cur + delay : lent[s] - 1;   // (cur + delay < lent, without the sum)
      plan->src_frame[row] = src * step + first;
      cur++;
    }
  }
}

// aslp-nnet-train-blstm-streams-lc.cc:215-245: a batch is chunk_size frames plus right_splice frames of right context per stream.  A live
// row takes frame and target `cur`, masked in only inside the chunk; a row behind the stream's end is zeros with the last target (none for
// a stream that never received an utterance) and mask 0.  Every cursor then moves on by chunk_size (the right context is read again as
// the head of the next chunk).
inline void PlanChunkBatch(int32 chunk_size, int32 right_splice, std::vector<int32> *curt, const std::vector<int32> &lent, StreamBatchPlan *plan) {
  const int32 S = (int32)lent.size(), B = chunk_size + right_splice;
  ASLP_ASSERT((int32)curt->size() == S && chunk_size >= 0 && right_splice >= 0);
  plan->Reset((size_t)B * S);
  if (AllStreamsDone(*curt, lent)) { plan->all_done = true; return; }
  for (int32 t = 0; t < B; t++) {
    for (int32 s = 0; s < S; s++) {
      const size_t row = (size_t)t * S + s;
      int32 &cur = (*curt)[s];
      if (cur < lent[s]) {
        plan->mask[row] = t >= chunk_size ? 0.0f : 1.0f;
        plan->tgt_index[row] = cur;
        plan->src_frame[row] = cur;
      } else if (lent[s] > 0) {
        plan->tgt_index[row] = lent[s] - 1;
      }
      cur++;
    }
  }
  for (int32 s = 0; s < S; s++) (*curt)[s] -= right_splice;
}

}  // namespace aslp
