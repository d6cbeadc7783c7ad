// nnet-loss.h -- Xent / Mse / MultiTaskLoss of the host engine.
// Same interface and Report() strings as src/aslp-nnet/nnet-loss.h:35-218 / nnet-loss.cc (the
// bash schedulers grep these lines).  `Posterior` is hmm/posterior.h's type.
// Difference in mechanism only: one fused kernel per Eval and NO blocking host reads per
// minibatch -- Xent's five statistics accumulate in device memory (double), Mse's per-row loss
// sums (and, where the weights are device-resident, its frame counts) are parked there batch by
// batch, and both are fetched when a report or the hourly progress line needs them.  Mse keeps
// the reference's op sequence behind ASLP_MSE_FUSED=0; MultiTaskLoss evaluates its tasks through
// Xent and Mse, an mse task straight into its column window of the diff; its device-resident form (EvalDevice) sends all xent tasks
// through one launch, aslp_xent_blocks_eval, which also stands in for a final <BlockSoftmax> (ASLP_MULTITASK_FUSED=0: the op sequence).
#pragma once
#include <string>
#include <utility>
#include <vector>

#include "cu-matrix.h"
#include "posterior.h"

namespace aslp {


class LossItf {
 public:
  virtual ~LossItf() {}
  virtual void Eval(const std::vector<BaseFloat> &frame_weights, const CuMatrixBase &net_out, const CuMatrixBase &target, CuMatrix *diff) = 0;
  virtual void Eval(const std::vector<BaseFloat> &frame_weights, const CuMatrixBase &net_out, const Posterior &target, CuMatrix *diff) = 0;
  virtual void Eval(const CuMatrixBase &net_out, const Posterior &target, CuMatrix *diff) {
    std::vector<BaseFloat> w(target.size(), 1.0f);
    Eval(w, net_out, target, diff);
  }
  virtual std::string Report() = 0;
  virtual BaseFloat AvgLoss() = 0;
};

void PosteriorToMatrix(const Posterior &post, int32 num_cols, CuMatrix *mat);  // nnet-utils.h:160-177

class Xent : public LossItf {
 public:
  Xent();
  void Eval(const std::vector<BaseFloat> &frame_weights, const CuMatrixBase &net_out, const CuMatrixBase &target, CuMatrix *diff);
  void Eval(const std::vector<BaseFloat> &frame_weights, const CuMatrixBase &net_out, const Posterior &target, CuMatrix *diff);
  using LossItf::Eval;
  // device-resident variants (no host data on the step path): weights / labels already on the GPU
  void EvalLabels(const CuVectorBase &frame_weights, const CuMatrixBase &net_out, const CuArray<int32> &labels, CuMatrix *diff);
  // `acts` are the activations in front of the network's final Softmax; the posteriors are formed inside the loss kernel
  // fw_max: the largest |frame weight| if the caller knows it (> 0): the diff's bound, which lets the kernel leave the diff's fp16 planes
  // for the layer product that reads it (csrc/split16.h)
  void EvalLabelsPreSoftmax(const CuVectorBase &frame_weights, const CuMatrixBase &acts, const int32 *labels_dev, CuMatrix *diff, float fw_max = -1.0f);
  void EvalLabels(const CuVectorBase &frame_weights, const CuMatrixBase &net_out, const int32 *labels_dev, CuMatrix *diff, float fw_max = -1.0f);
  // Eval(frame_weights, net_out, Posterior) for callers that hold the executor's buffers (Nnet::PropagateForLoss):
  // `loss_input` is the network output, or the activations in front of its final Softmax when `pre_softmax`
  void EvalOnLossInput(const std::vector<BaseFloat> &frame_weights, const CuMatrixBase &loss_input, bool pre_softmax, const Posterior &target,
                       CuMatrix *diff);
  // Soft targets as the sparse object they are: CSR in device memory (row_begin [rows + 1], columns strictly increasing within a row,
  // weights; include/aslp_kernels.h: aslp_xent_sparse_eval).  One launch, the row statistics deferred as on the label path; the bits of
  // Eval(frame_weights, net_out, <dense matrix of the same entries>, diff).  `loss_input` as for EvalOnLossInput.
  void EvalSparse(const CuVectorBase &frame_weights, const CuMatrixBase &loss_input, bool pre_softmax, const int32 *row_begin_dev,
                  const int32 *col_dev, const float *w_dev, CuMatrix *diff);
  // ... into a matrix the caller owns (not resized: a C ABI caller's buffer)
  void EvalSparseInto(const CuVectorBase &frame_weights, const CuMatrixBase &loss_input, bool pre_softmax, const int32 *row_begin_dev,
                      const int32 *col_dev, const float *w_dev, CuMatrixBase *diff);
  // The A/B switch of the Posterior route (ASLP_XENT_SPARSE=0, read once per process; aslp_xent_sparse): off = PosteriorToMatrix and the
  // dense kernel, as before.  EvalSparse itself is not switched.
  static bool Sparse();
  static void SetSparse(bool on);
  std::string Report();
  BaseFloat AvgLoss() { Fetch(); return (loss_ - entropy_) / frames_; }
  // raw accumulators {frames, correct, loss, entropy, likelyhood}
  void GetStats(double out[5]) { Fetch(); out[0] = frames_; out[1] = correct_; out[2] = loss_; out[3] = entropy_; out[4] = likelyhood_; }
  // For a kernel that evaluates this Xent beside others in one launch (MultiTaskLoss::EvalDevice): DeferredRoom gives the room for the
  // batch's [rows x 5] row statistics (NULL: too many rows to defer -- the caller keeps them itself and hands them to AddRowStats);
  // EvalDone is the bookkeeping behind every evaluated batch.
  double *DeferredRoom(int32 rows) { return PendingRowStats(rows); }
  void AddRowStats(const double *rowstats, int32 rows);
  void EvalDone(int32 rows) { AfterEval(rows); }

 private:
  void Fetch();
  void AfterEval(int rows);
  double frames_, correct_, loss_, entropy_, likelyhood_;
  double frames_progress_, loss_progress_, entropy_progress_, likelyhood_progress_;
  double rows_since_progress_;
  std::vector<float> loss_vec_;
  CuVector frame_weights_;
  CuMatrix tgt_mat_;
  CuArray<int32> labels_;
  // a non-one-hot Posterior as CSR under PosteriorToMatrix' rules, in one buffer {row_begin [rows + 1], columns [nnz], weights' bits [nnz]}:
  // built in csr_host_, sent with one copy into csr_ (both grow, neither shrinks).  frame_weights_ holds the batch's weights.
  void EvalPosteriorSparse(const CuMatrixBase &loss_input, bool pre_softmax, const Posterior &post, CuMatrix *diff);
  std::vector<int32> csr_host_;
  CuArray<int32> csr_;
  CuVectorD stats_;  // device accumulators
  bool dirty_;
  // The label-target evaluations (the step path) leave their per-row statistics here, batch after batch, and the sum into stats_ is made
  // for all of them at once when the room is used up or the accumulators are read (Fetch): same bits, one launch less per step.
  double *PendingRowStats(int32 rows);   // room for the next batch's [rows x 5], or NULL: too large to defer
  void FlushPending();
  CuVectorD pending_;
  int32 pending_rows_ = 0, pending_batches_ = 0, pending_cap_ = 0;
};

// One launch per Eval (aslp_mse_eval): the diff, the per-row loss sums and the per-workgroup maxima of |diff|.  The row sums are parked
// batch after batch and reach loss_ -- 0.5 * sum per minibatch, in batch order, with the reference's progress line -- when AvgLoss(),
// Report(), GetStats() or that progress line needs them (Fetch).  ASLP_MSE_FUSED=0 (read once per process): the reference's op sequence.
class Mse : public LossItf {
 public:
  Mse() : frames_(0.0), loss_(0.0), frames_progress_(0.0), loss_progress_(0.0), num_tgt_(0) {}
  void Eval(const std::vector<BaseFloat> &frame_weights, const CuMatrixBase &net_out, const CuMatrixBase &target, CuMatrix *diff);
  void Eval(const std::vector<BaseFloat> &frame_weights, const CuMatrixBase &net_out, const Posterior &target, CuMatrix *diff);
  using LossItf::Eval;
  // device-resident variant (no host data on the step path): weights and targets already on the GPU.  The minibatch's frame count
  // (int32 of the weights' sum) is formed on the device and fetched with the losses.
  void EvalDevice(const CuVectorBase &frame_weights, const CuMatrixBase &net_out, const CuMatrixBase &target, CuMatrix *diff);
  // Eval / EvalDevice into a matrix the caller owns (not resized: a column window of MultiTaskLoss' diff, a C ABI caller's buffer), the
  // diff multiplied by `scale` as a second rounding (MultiTaskLoss' task weight).  frame_weights == NULL: the device variant.
  void EvalInto(const std::vector<BaseFloat> *frame_weights, const CuVectorBase *frame_weights_dev, const CuMatrixBase &net_out,
                const CuMatrixBase &target, CuMatrixBase *diff, BaseFloat scale);
  static bool Fused();   // the A/B switch
  std::string Report();
  BaseFloat AvgLoss() { Fetch(); return loss_ / frames_; }
  // raw accumulators {frames, loss, num_tgt}
  void GetStats(double out[3]) { Fetch(); out[0] = frames_; out[1] = loss_; out[2] = num_tgt_; }

 private:
  void EvalOps(const std::vector<BaseFloat> &frame_weights, const CuMatrixBase &net_out, const CuMatrixBase &target, CuMatrix *diff);
  void AddBatch(double mean_square_error, double num_frames);   // one minibatch into the accumulators (nnet-loss.cc:240-257)
  double *PendingRoom(int32 rows);   // room for the next batch's rows + 1 doubles
  void FlushPending();               // parked rows -> one {sum, frames} pair per batch in sums_ (one launch)
  void DrainSums();                  // ... -> the host accumulators, batch by batch (the one blocking read)
  void Fetch();                      // both
  double frames_, loss_, frames_progress_, loss_progress_;
  std::vector<float> loss_vec_;
  CuVector frame_weights_;
  CuMatrix tgt_mat_;
  int num_tgt_;
  CuVectorD pending_, sums_;
  int32 pending_rows_ = 0, pending_batches_ = 0, pending_cap_ = 0, num_sums_ = 0;
  std::vector<double> host_frames_;   // per parked batch: the frame count the host formed, or -1 = the device's
  double parked_frames_ = 0.0;        // of the parked batches: frames (rows where only the device knows) since the last Fetch
};

class MultiTaskLoss : public LossItf {
 public:
  MultiTaskLoss() {}
  ~MultiTaskLoss() { for (LossItf *l : loss_vec_) delete l; }
  void InitFromString(const std::string &s);
  void Eval(const std::vector<BaseFloat> &, const CuMatrixBase &, const CuMatrixBase &, CuMatrix *) { ASLP_ERR << "This is not supposed to be called!"; }
  void Eval(const std::vector<BaseFloat> &frame_weights, const CuMatrixBase &net_out, const Posterior &target, CuMatrix *diff);
  using LossItf::Eval;
  // Device-resident variant (no host data on the step path).  `loss_input` [rows x sum of the task dims] is the network output or, with
  // `pre_block_softmax`, the activations in front of a <BlockSoftmax> whose blocks are the tasks (all xent): the kernel then forms the
  // posteriors and applies the component's backward mask.  labels_dev: [rows x number of xent tasks] in task order, relative to the task's
  // first column, < 0 = no target.  dense_targets (NULL without an mse task): full width, read in the mse tasks' windows only.
  // All xent tasks go through one aslp_xent_blocks_eval, their row statistics into each task's own Xent; an mse task through
  // Mse::EvalInto into its window.  `diff` is the caller's [rows x cols].  With the switch off (Fused()): the op sequence of Eval above --
  // dense targets scattered from the labels, per task Eval, Scale, CopyFromMat -- and no pre_block_softmax.
  void EvalDevice(const CuVectorBase &frame_weights, const CuMatrixBase &loss_input, bool pre_block_softmax, const int32 *labels_dev,
                  const CuMatrixBase *dense_targets, CuMatrixBase *diff);
  static bool Fused();            // the A/B switch: ASLP_MULTITASK_FUSED=0, or SetFused(false)
  static void SetFused(bool on);
  std::string Report();
  BaseFloat AvgLoss();
  // the task table
  enum TaskKind { kXentTask = 0, kMseTask = 1 };
  int32 NumTasks() const { return (int32)loss_vec_.size(); }
  int32 NumXentTasks() const;
  TaskKind Kind(int32 task) const;
  int32 Dim(int32 task) const { return loss_dim_[task]; }
  int32 Offset(int32 task) const { return loss_dim_offset_[task]; }
  int32 TotalDim() const { return loss_dim_offset_.back(); }
  BaseFloat Weight(int32 task) const { return loss_weights_[task]; }
  // a task's raw accumulators: Xent::GetStats' five, or Mse::GetStats' three followed by two zeros
  void GetTaskStats(int32 task, double out[5]);

 private:
  void EvalTasks(const std::vector<BaseFloat> &frame_weights, const CuMatrixBase &net_out, CuMatrixBase *diff);   // from tgt_mat_
  CuVectorD rowstats_tmp_;
  std::vector<LossItf *> loss_vec_;
  std::vector<int32> loss_dim_;
  std::vector<BaseFloat> loss_weights_;
  std::vector<int32> loss_dim_offset_;
  CuMatrix tgt_mat_;
};

}  // namespace aslp
