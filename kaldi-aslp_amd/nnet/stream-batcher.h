// stream-batcher.h -- multi-stream batches built in device memory ("Stream batches gathered on the device").
// Every stream's current utterance -- its features as the feature transform left them -- stays on the device in a buffer of the stream's
// own; a batch is one gather launch (aslp_gather_stream_rows) driven by a plan of source rows that the host computes (stream-batch-plan.h)
// and uploads through the small staging slots.  Nothing on this path waits for the device.  The targets stay on the host as they come from
// the table; beside them the batcher keeps one label per frame where the frame's posterior is one-hot, so that a batch of one-hot targets
// reaches the loss as an array of labels without a Posterior being copied row by row.
#pragma once
#include <utility>
#include <vector>

#include "cu-matrix.h"
#include "posterior.h"
#include "stream-batch-plan.h"

namespace aslp {

class StreamBatcher {
 public:
  explicit StreamBatcher(int32 num_stream)
      : bufs_(num_stream), table_(num_stream), targets_(num_stream), labels_(num_stream), curt_(num_stream, 0), lent_(num_stream, 0),
        table_dirty_(true) {
    for (auto &t : table_) { t.base = nullptr; t.stride = 0; t.rows = 0; }
  }
  int32 NumStreams() const { return (int32)bufs_.size(); }
  // the buffers grow in steps of 1024 rows and never shrink (like MatrixRandomizer::GrownRows: the allocator keeps one block per distinct
  // size, and utterance lengths are all distinct)
  static int32 GrownRows(int32 need) { return (need + 1023) / 1024 * 1024; }

  // Stream s takes a new utterance: its features (on the device already: the transform's output; or on the host: sent through the staged
  // upload) and its targets.  With skip_width > 1 the stream trains on the frames skip_offset, skip_offset + skip_width, ... only; the
  // features are kept whole (the plan picks the rows), the targets are thinned here.
  void SetUtterance(int32 s, const CuMatrixBase &feats, const Posterior &targets, int32 skip_width = 1, int32 skip_offset = 0) {
    Room(s, feats.NumRows(), feats.NumCols());
    if (feats.NumRows() > 0) bufs_[s].RowRange(0, feats.NumRows()).CopyFromMat(feats);
    SetTargets(s, feats.NumRows(), targets, skip_width, skip_offset);
  }
  void SetUtterance(int32 s, const HostMatrix &feats, const Posterior &targets, int32 skip_width = 1, int32 skip_offset = 0) {
    Room(s, feats.rows, feats.cols);
    if (feats.rows > 0) bufs_[s].RowRange(0, feats.rows).CopyFromMat(feats);
    SetTargets(s, feats.rows, targets, skip_width, skip_offset);
  }
  bool StreamDone(int32 s) const { return curt_[s] >= lent_[s]; }
  bool AllDone() const { return AllStreamsDone(curt_, lent_); }
  int32 Cols(int32 s) const { return bufs_[s].NumCols(); }
  const StreamBatchPlan &Plan() const { return plan_; }

  // SequenceDataReader's batch (PlanSequenceBatch).  false: every stream was exhausted, *feat is as it was and the mask is all zero.
  // A row without a target of its own (its stream never received an utterance, or one that skipping left no frame of) keeps the target
  // the row had in the batch before, as it does in the host assembly, which leaves that element of the caller's Posterior alone.
  bool SequenceBatch(int32 B, int32 delay, int32 skip_width, int32 skip_offset, CuMatrix *feat) {
    PlanSequenceBatch(B, delay, skip_width, skip_offset, &curt_, lent_, &plan_);
    BookTargets(true);
    if (plan_.all_done) return false;
    Gather(B, Cols(0), feat);
    return true;
  }
  // the latency-controlled tools' batch (PlanChunkBatch); a row without a target has an empty one
  bool ChunkBatch(int32 chunk_size, int32 right_splice, int32 feat_dim, CuMatrix *feat) {
    PlanChunkBatch(chunk_size, right_splice, &curt_, lent_, &plan_);
    if (plan_.all_done) return false;
    BookTargets(false);
    Gather(chunk_size + right_splice, feat_dim, feat);
    return true;
  }
  // the targets of the batch planned last, as the host assembly hands them out
  void BatchTargets(Posterior *target) const {
    target->resize(row_label_.size());
    for (size_t row = 0; row < row_label_.size(); row++) {
      if (row_label_[row] >= 0) (*target)[row].assign(1, std::make_pair(row_label_[row], 1.0f));
      else (*target)[row] = row_post_[row];
    }
  }
  // ... and as labels, when every row's target is one-hot in the sense of Xent::Eval (one pair, weight 1, label >= 0): true, and *labels
  // is filled.  A label >= num_pdf is the error it is there.
  bool BatchLabels(int32 num_pdf, std::vector<int32> *labels) const {
    if (!all_one_hot_) return false;
    for (int32 l : row_label_)
      if (l >= num_pdf) ASLP_ERR << "Out-of-bound Posterior element with index " << l << ", higher than number of columns " << num_pdf;
    *labels = row_label_;
    return true;
  }
  // the label Xent::Eval would take from one frame's posterior, -1 where it would not
  static int32 OneHotLabel(const Posterior::value_type &p) {
    return p.size() == 1 && p[0].second == 1.0f && p[0].first >= 0 ? p[0].first : -1;
  }

 private:
  void Room(int32 s, int32 rows, int32 cols) {
    CuMatrix &b = bufs_[s];
    if (b.NumCols() != cols || b.NumRows() < rows) b.Resize(GrownRows(rows), cols, kUndefined);
    if (table_[s].base != b.Data() || table_[s].stride != b.Stride() || table_[s].rows != rows) table_dirty_ = true;
    table_[s].base = b.Data();
    table_[s].stride = b.Stride();
    table_[s].rows = rows;
  }
  void SetTargets(int32 s, int32 rows, const Posterior &targets, int32 skip_width, int32 skip_offset) {
    ASLP_ASSERT(rows == (int32)targets.size());
    if (skip_width > 1) {
      const int32 skip_len = rows > skip_offset ? (rows - 1 - skip_offset) / skip_width + 1 : 0;
      targets_[s].assign(skip_len, Posterior::value_type());
      for (int32 i = 0; i < skip_len; i++) targets_[s][i] = targets[(size_t)i * skip_width + skip_offset];
    } else {
      targets_[s] = targets;
    }
    labels_[s].resize(targets_[s].size());
    for (size_t i = 0; i < targets_[s].size(); i++) labels_[s][i] = OneHotLabel(targets_[s][i]);
    curt_[s] = 0;
    lent_[s] = (int32)targets_[s].size();
  }
  // per row of the planned batch: its label where the target is one-hot, the target itself where it is not
  void BookTargets(bool keep_stale) {
    const int32 S = NumStreams();
    const size_t rows = plan_.tgt_index.size();
    row_label_.resize(rows, -1);
    row_post_.resize(rows);
    all_one_hot_ = rows > 0;
    for (size_t row = 0; row < rows; row++) {
      const int32 s = (int32)(row % S), i = plan_.tgt_index[row];
      if (i >= 0) {
        row_label_[row] = labels_[s][i];
        if (row_label_[row] < 0) row_post_[row] = targets_[s][i];
      } else if (!keep_stale) {
        row_label_[row] = -1;
        row_post_[row].clear();
      }
      if (row_label_[row] < 0) all_one_hot_ = false;
    }
  }
  void Gather(int32 B, int32 D, CuMatrix *feat) {
    const int32 S = NumStreams();
    if (table_dirty_) {
      table_dev_.CopyFromVec(table_);
      table_dirty_ = false;
    }
    plan_dev_.CopyFromVec(plan_.src_frame);
    feat->Resize(B * S, D, kUndefined);
    if (aslp_gather_stream_rows(feat->Data(), feat->Stride(), B, S, D, table_.data(), table_dev_.Data(), plan_.src_frame.data(), plan_dev_.Data()))
      CheckKernelError();
    CheckKernelError();
  }
  std::vector<CuMatrix> bufs_;
  std::vector<aslp_stream_src> table_;
  std::vector<Posterior> targets_;
  std::vector<std::vector<int32>> labels_;
  std::vector<int32> curt_, lent_;
  StreamBatchPlan plan_;
  std::vector<int32> row_label_;
  Posterior row_post_;
  bool all_one_hot_ = false;
  CuArray<aslp_stream_src> table_dev_;
  CuArray<int32> plan_dev_;
  bool table_dirty_;
};

}  // namespace aslp
