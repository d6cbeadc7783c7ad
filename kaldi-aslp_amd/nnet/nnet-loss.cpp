// nnet-loss.cpp -- follows src/aslp-nnet/nnet-loss.cc (line cited per function).
#include "nnet-loss.h"
#include "split16.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>

namespace aslp {

static void CheckK() {
  char buf[512];
  if (aslp_get_last_error(buf, sizeof(buf))) ASLP_ERR << buf;
}

void PosteriorToMatrix(const Posterior &post, int32 num_cols, CuMatrix *mat) {
  // nnet-utils.h:160-177: zero matrix, m(t, col) = weight (assignment: a later duplicate wins)
  int32 num_rows = post.size();
  mat->Resize(num_rows, num_cols, kSetZero);
  std::vector<int32> rows, cols;
  std::vector<float> vals;
  for (int32 t = 0; t < num_rows; t++) {
    std::map<int32, float> last;
    for (size_t i = 0; i < post[t].size(); i++) {
      int32 col = post[t][i].first;
      if (col >= num_cols) ASLP_ERR << "Out-of-bound Posterior element with index " << col << ", higher than number of columns " << num_cols;
      last[col] = post[t][i].second;
    }
    for (auto &kv : last) { rows.push_back(t); cols.push_back(kv.first); vals.push_back(kv.second); }
  }
  if (rows.empty()) return;
  CuArray<int32> r(rows), c(cols);
  CuVector v;
  HostVector hv;
  hv.data = vals;
  v = hv;
  aslp_scatter_add(mat->Data(), mat->Dim(), r.Data(), c.Data(), v.Data(), (int)rows.size());
  CheckK();
}

Xent::Xent()
    : frames_(0.0), correct_(0.0), loss_(0.0), entropy_(0.0), likelyhood_(0.0), frames_progress_(0.0), loss_progress_(0.0),
      entropy_progress_(0.0), likelyhood_progress_(0.0), rows_since_progress_(0.0), dirty_(false) {
  stats_.Resize(5, kSetZero);
}

double *Xent::PendingRowStats(int32 rows) {
  static const int32 kMaxBatches = 32, kMaxRows = 1 << 16;
  if (rows != pending_rows_) {
    FlushPending();
    pending_rows_ = rows;
    pending_cap_ = std::min(kMaxBatches, kMaxRows / std::max(rows, 1));
    if (pending_cap_ >= 2 && pending_.Dim() < pending_cap_ * rows * 5) pending_.Resize(pending_cap_ * rows * 5, kUndefined);
  }
  if (pending_cap_ < 2) return nullptr;
  if (pending_batches_ == pending_cap_) FlushPending();
  return pending_.Data() + (size_t)(pending_batches_++) * rows * 5;
}
void Xent::FlushPending() {
  if (pending_batches_ > 0) aslp_xent_sum_rowstats(pending_.Data(), pending_rows_, pending_batches_, stats_.Data());
  pending_batches_ = 0;
}

void Xent::Fetch() {
  if (!dirty_) return;
  FlushPending();
  double h[5];
  stats_.CopyToHost(h);
  stats_.SetZero();
  dirty_ = false;
  if (!std::isfinite(h[2])) ASLP_ERR << "Xent: cross-entropy is not finite";    // nnet-loss.cc:124-126
  if (!std::isfinite(h[3])) ASLP_ERR << "Xent: target entropy is not finite";
  if (!std::isfinite(h[4])) ASLP_ERR << "Xent: likelihood is not finite";
  frames_ += h[0]; correct_ += h[1]; loss_ += h[2]; entropy_ += h[3]; likelyhood_ += h[4];
  frames_progress_ += h[0]; loss_progress_ += h[2]; entropy_progress_ += h[3]; likelyhood_progress_ += h[4];
}

void Xent::AfterEval(int rows) {
  dirty_ = true;
  // progressive loss reporting (nnet-loss.cc:134-155): every 1h of frames.  The frame count is
  // only known on the device, so the row count gates the (rare) fetch.
  static const int32 progress_step = 3600 * 100;
  rows_since_progress_ += rows;
  if (rows_since_progress_ > progress_step) {
    Fetch();
    if (frames_progress_ > progress_step) {
      ASLP_LOG << "ProgressLoss[last " << static_cast<int>(frames_progress_ / 100 / 3600) << "h of "
               << static_cast<int>(frames_ / 100 / 3600) << "h]: " << likelyhood_progress_ / frames_progress_ << " (Likelyhood) "
               << (loss_progress_ - entropy_progress_) / frames_progress_ << " (Xent)";
      loss_vec_.push_back((loss_progress_ - entropy_progress_) / frames_progress_);
      frames_progress_ = 0; loss_progress_ = 0.0; entropy_progress_ = 0.0; likelyhood_progress_ = 0.0;
      rows_since_progress_ = 0;
    }
  }
}

void Xent::Eval(const std::vector<BaseFloat> &frame_weights, const CuMatrixBase &net_out, const CuMatrixBase &targets, CuMatrix *diff) {
  // nnet-loss.cc:63-156
  ASLP_ASSERT(net_out.NumCols() == targets.NumCols());
  ASLP_ASSERT(net_out.NumRows() == targets.NumRows());
  ASLP_ASSERT(net_out.NumRows() == (int)frame_weights.size());
  for (BaseFloat w : frame_weights) ASLP_ASSERT(std::isfinite(w));
  HostVector hv;
  hv.data = frame_weights;
  frame_weights_ = hv;
  diff->Resize(net_out.NumRows(), net_out.NumCols(), kUndefined);
  FlushPending();   // (the accumulators take the batches in evaluation order)
  aslp_xent_eval(net_out.Data(), net_out.Dim(), targets.Data(), targets.Stride(), nullptr, frame_weights_.Data(), diff->Data(),
                 diff->Stride(), stats_.Data());
  CheckK();
  AfterEval(net_out.NumRows());
}

void Xent::Eval(const std::vector<BaseFloat> &frame_weights, const CuMatrixBase &net_out, const Posterior &post, CuMatrix *diff) {
  // nnet-loss.cc:159-172.  One-hot posteriors (the normal alignment case) skip the dense
  // [frames x pdfs] target matrix: the fused kernel takes the label directly.
  int32 num_frames = net_out.NumRows(), num_pdf = net_out.NumCols();
  ASLP_ASSERT(num_frames == (int32)post.size());
  bool one_hot = true;
  std::vector<int32> labels(num_frames);
  for (int32 t = 0; t < num_frames && one_hot; t++) {
    if (post[t].size() != 1 || post[t][0].second != 1.0f) one_hot = false;
    else {
      labels[t] = post[t][0].first;
      if (labels[t] >= num_pdf) ASLP_ERR << "Out-of-bound Posterior element with index " << labels[t] << ", higher than number of columns " << num_pdf;
      if (labels[t] < 0) one_hot = false;
    }
  }
  if (!one_hot) {
    if (Sparse() && aslp_xent_sparse_supported(num_pdf, 0)) {   // soft targets stay sparse: no dense matrix is built
      ASLP_ASSERT(num_frames == (int)frame_weights.size());
      for (BaseFloat w : frame_weights) ASLP_ASSERT(std::isfinite(w));
      HostVector hv;
      hv.data = frame_weights;
      frame_weights_ = hv;
      EvalPosteriorSparse(net_out, false, post, diff);
      return;
    }
    PosteriorToMatrix(post, num_pdf, &tgt_mat_);
    Eval(frame_weights, net_out, tgt_mat_, diff);
    return;
  }
  ASLP_ASSERT(num_frames == (int)frame_weights.size());
  HostVector hv;
  hv.data = frame_weights;
  frame_weights_ = hv;
  labels_ = labels;
  EvalLabels(frame_weights_, net_out, labels_, diff);
}

// Xent with one label per frame.  On posteriors |diff| = |y - t| w <= max w, known before the launch when the caller knows its frame
// weights' maximum (fw_max > 0).  If the network asked for the diff's planes (Nnet::LossDiff -> s16_loss_diff_target) the kernel
// writes them beside the diff.
static void XentLabels(const CuMatrixBase &in, bool softmax, const int32 *labels_dev, const CuVectorBase &fw, float fw_max, CuMatrix *diff,
                       double *stats, double *rowstats_room) {
  S16DiffTarget t = s16_loss_diff_target();
  s16_loss_diff_target() = S16DiffTarget();
  aslp_planes_out po = aslp_planes_out();
  // (only where the kernel forms the posteriors itself: what a caller hands in as "net_out" need not be posteriors -- a linear output
  //  layer -- and |y - t| <= 1 is then nobody's promise; the consumer of the diff converts it with a measured maximum instead)
  PlaneSet *ps = (softmax && t.planes && t.diff == diff->Data() && fw_max > 0.0f && std::isfinite(fw_max)) ? t.planes : nullptr;
  if (ps && ps->Reserve(in.NumRows(), in.NumCols()) && ps->SetBound(fw_max)) aslp_planes_as_output(reinterpret_cast<const aslp_planes *>(ps), &po);
  else ps = nullptr;
  const int planes = rowstats_room
                         ? aslp_xent_eval_rows(in.Data(), in.Dim(), labels_dev, fw.Data(), diff->Data(), diff->Stride(), rowstats_room, softmax ? 1 : 0, ps ? &po : nullptr)
                         : aslp_xent_eval_p(in.Data(), in.Dim(), labels_dev, fw.Data(), diff->Data(), diff->Stride(), stats, softmax ? 1 : 0, ps ? &po : nullptr);
  if (planes && ps) ps->Tag(diff->Data(), diff->Stride(), t.epoch);
}

void Xent::EvalLabels(const CuVectorBase &fw, const CuMatrixBase &net_out, const CuArray<int32> &labels, CuMatrix *diff) {
  ASLP_ASSERT(fw.Dim() == net_out.NumRows() && labels.Dim() == net_out.NumRows());
  diff->Resize(net_out.NumRows(), net_out.NumCols(), kUndefined);
  FlushPending();
  aslp_xent_eval(net_out.Data(), net_out.Dim(), nullptr, 0, labels.Data(), fw.Data(), diff->Data(), diff->Stride(), stats_.Data());
  CheckK();
  AfterEval(net_out.NumRows());
}

void Xent::EvalLabels(const CuVectorBase &fw, const CuMatrixBase &net_out, const int32 *labels_dev, CuMatrix *diff, float fw_max) {
  ASLP_ASSERT(fw.Dim() == net_out.NumRows());
  diff->Resize(net_out.NumRows(), net_out.NumCols(), kUndefined);
  XentLabels(net_out, false, labels_dev, fw, fw_max, diff, stats_.Data(), PendingRowStats(net_out.NumRows()));
  CheckK();
  AfterEval(net_out.NumRows());
}
void Xent::EvalLabelsPreSoftmax(const CuVectorBase &fw, const CuMatrixBase &acts, const int32 *labels_dev, CuMatrix *diff, float fw_max) {
  ASLP_ASSERT(fw.Dim() == acts.NumRows());
  diff->Resize(acts.NumRows(), acts.NumCols(), kUndefined);
  if (!aslp_softmax_xent_supported(acts.NumCols())) ASLP_ERR << "Softmax + Xent in one pass: unsupported number of classes " << acts.NumCols();
  XentLabels(acts, true, labels_dev, fw, fw_max, diff, stats_.Data(), PendingRowStats(acts.NumRows()));
  CheckK();
  AfterEval(acts.NumRows());
}

void Xent::EvalOnLossInput(const std::vector<BaseFloat> &frame_weights, const CuMatrixBase &in, bool pre_softmax, const Posterior &post,
                           CuMatrix *diff) {
  if (!pre_softmax) { Eval(frame_weights, in, post, diff); return; }
  const int32 num_frames = in.NumRows(), num_pdf = in.NumCols();
  ASLP_ASSERT(num_frames == (int32)post.size() && num_frames == (int32)frame_weights.size());
  for (BaseFloat w : frame_weights) ASLP_ASSERT(std::isfinite(w));
  bool one_hot = true;
  std::vector<int32> labels(num_frames);
  for (int32 t = 0; t < num_frames && one_hot; t++) {
    if (post[t].size() != 1 || post[t][0].second != 1.0f || post[t][0].first < 0) one_hot = false;
    else {
      labels[t] = post[t][0].first;
      if (labels[t] >= num_pdf) ASLP_ERR << "Out-of-bound Posterior element with index " << labels[t] << ", higher than number of columns " << num_pdf;
    }
  }
  HostVector hv;
  hv.data = frame_weights;
  frame_weights_ = hv;
  diff->Resize(num_frames, num_pdf, kUndefined);
  if (one_hot) {
    labels_ = labels;
    float fw_max = 0.0f;
    for (BaseFloat w : frame_weights) fw_max = std::max(fw_max, std::fabs(w));
    XentLabels(in, true, labels_.Data(), frame_weights_, fw_max, diff, stats_.Data(), PendingRowStats(num_frames));
  } else if (Sparse() && aslp_xent_sparse_supported(num_pdf, 1)) {
    EvalPosteriorSparse(in, true, post, diff);   // (does the bookkeeping itself)
    return;
  } else {
    PosteriorToMatrix(post, num_pdf, &tgt_mat_);
    FlushPending();
    aslp_softmax_xent_eval(in.Data(), in.Dim(), tgt_mat_.Data(), tgt_mat_.Stride(), nullptr, frame_weights_.Data(), diff->Data(), diff->Stride(),
                           stats_.Data(), nullptr, 0);
  }
  CheckK();
  AfterEval(num_frames);
}

static int g_xent_sparse = -1;   // -1: not asked yet (the environment decides)
bool Xent::Sparse() {
  if (g_xent_sparse < 0) {
    const char *e = getenv("ASLP_XENT_SPARSE");
    g_xent_sparse = (e != nullptr && e[0] == '0') ? 0 : 1;
  }
  return g_xent_sparse != 0;
}
void Xent::SetSparse(bool on) { g_xent_sparse = on ? 1 : 0; }

void Xent::EvalSparseInto(const CuVectorBase &fw, const CuMatrixBase &in, bool pre_softmax, const int32 *row_begin_dev, const int32 *col_dev,
                          const float *w_dev, CuMatrixBase *diff) {
  ASLP_ASSERT(fw.Dim() == in.NumRows() && diff->NumRows() == in.NumRows() && diff->NumCols() == in.NumCols());
  if (!aslp_xent_sparse_supported(in.NumCols(), pre_softmax ? 1 : 0))
    ASLP_ERR << "Xent on sparse targets" << (pre_softmax ? " with the Softmax" : "") << ": unsupported number of classes " << in.NumCols();
  double *room = PendingRowStats(in.NumRows());
  if (room) aslp_xent_sparse_eval_rows(in.Data(), in.Dim(), row_begin_dev, col_dev, w_dev, fw.Data(), diff->Data(), diff->Stride(), room,
                                       pre_softmax ? 1 : 0, nullptr, 0);
  else aslp_xent_sparse_eval(in.Data(), in.Dim(), row_begin_dev, col_dev, w_dev, fw.Data(), diff->Data(), diff->Stride(), stats_.Data(),
                             pre_softmax ? 1 : 0, nullptr, 0);
  CheckK();
  AfterEval(in.NumRows());
}
void Xent::EvalSparse(const CuVectorBase &fw, const CuMatrixBase &in, bool pre_softmax, const int32 *row_begin_dev, const int32 *col_dev,
                      const float *w_dev, CuMatrix *diff) {
  diff->Resize(in.NumRows(), in.NumCols(), kUndefined);
  EvalSparseInto(fw, in, pre_softmax, row_begin_dev, col_dev, w_dev, diff);
}

void Xent::EvalPosteriorSparse(const CuMatrixBase &in, bool pre_softmax, const Posterior &post, CuMatrix *diff) {
  // PosteriorToMatrix' rules (nnet-utils.h:160-177 and the scatter behind it): a later duplicate of a column wins, a column >= num_cols is an
  // error, a negative one is dropped; the columns sorted within the row
  const int32 rows = in.NumRows(), num_cols = in.NumCols();
  ASLP_ASSERT(rows == (int32)post.size());
  size_t cap = 0;
  for (int32 t = 0; t < rows; t++) cap += post[t].size();
  std::vector<int32> &h = csr_host_;
  if (h.size() < (size_t)rows + 1 + 2 * cap) h.resize((size_t)rows + 1 + 2 * cap);
  std::vector<std::pair<int32, BaseFloat>> row;
  // (columns and weights are laid out behind row_begin once nnz is known: first gathered at the width `cap`)
  int32 *rb = h.data(), *col = rb + rows + 1, *wb = col + cap;
  int32 nnz = 0;
  rb[0] = 0;
  for (int32 t = 0; t < rows; t++) {
    row.clear();
    for (size_t i = 0; i < post[t].size(); i++) {
      const int32 c = post[t][i].first;
      if (c >= num_cols) ASLP_ERR << "Out-of-bound Posterior element with index " << c << ", higher than number of columns " << num_cols;
      if (c < 0) continue;
      size_t j = 0;
      while (j < row.size() && row[j].first != c) j++;
      if (j < row.size()) row[j].second = post[t][i].second;
      else row.push_back(std::make_pair(c, post[t][i].second));
    }
    std::sort(row.begin(), row.end(), [](const std::pair<int32, BaseFloat> &a, const std::pair<int32, BaseFloat> &b) { return a.first < b.first; });
    for (size_t j = 0; j < row.size(); j++, nnz++) {
      col[nnz] = row[j].first;
      std::memcpy(wb + nnz, &row[j].second, sizeof(float));
    }
    rb[t + 1] = nnz;
  }
  if ((size_t)nnz < cap) std::memmove(col + nnz, wb, sizeof(int32) * (size_t)nnz);   // the weights right behind the columns
  const int32 total = rows + 1 + 2 * nnz;
  if (csr_.Dim() < total) csr_.Resize(std::max(total, 2 * csr_.Dim()));
  // One buffer, sent in pieces of at most 16000 bytes: a copy above 16 KB leaves the runtime's copy kernel for the DMA engine, whose
  // hand-over to the compute queue and back cost 0.06 ms per step at minibatch 1024 (29 KB in one copy: measured).
  static const int32 kPiece = 4000;
  for (int32 o = 0; o < total; o += kPiece) HostToDevice(csr_.Data() + o, h.data() + o, sizeof(int32) * (size_t)std::min(kPiece, total - o));
  const int32 *dev = csr_.Data();
  EvalSparse(frame_weights_, in, pre_softmax, dev, dev + rows + 1, reinterpret_cast<const float *>(dev + rows + 1 + nnz), diff);
}

std::string Xent::Report() {  // nnet-loss.cc:175-199
  Fetch();
  std::ostringstream oss;
  if (0 == frames_) {
    oss << "AvgLoss: " << 0.0 << " (Xent), " << "Likelyhood: " << 0.0 << " " << "Frame: " << 0 << std::endl;
    oss << "FRAME_ACCURACY >> " << 0.0 << "% <<" << std::endl;
  } else {
    oss << "AvgLoss: " << (loss_ - entropy_) / frames_ << " (Xent), " << "Likelyhood: " << (likelyhood_) / frames_ << " "
        << "Frame: " << frames_ << std::endl;
    if (correct_ >= 0.0) oss << "FRAME_ACCURACY >> " << 100.0 * correct_ / frames_ << "% <<" << std::endl;
  }
  return oss.str();
}

bool Mse::Fused() {
  static const bool off = [] { const char *e = getenv("ASLP_MSE_FUSED"); return e != nullptr && e[0] == '0'; }();   // A/B switch
  return !off;
}

// the frame count of a minibatch as the reference forms it: the weights summed in double, truncated (nnet-loss.cc:216-219)
static int32 MseNumFrames(const std::vector<BaseFloat> &frame_weights) {
  double fsum = 0.0;
  for (BaseFloat w : frame_weights) fsum += w;
  ASLP_ASSERT(std::isfinite(fsum));
  int32 num_frames = fsum;
  ASLP_ASSERT(num_frames >= 0.0);
  return num_frames;
}

void Mse::AddBatch(double mean_square_error, double num_frames) {   // nnet-loss.cc:240-257
  if (!std::isfinite(mean_square_error)) ASLP_ERR << "Mse: mean square error is not finite";
  loss_ += mean_square_error;
  frames_ += num_frames;
  static const int32 progress_step = 3600 * 100;
  frames_progress_ += num_frames;
  loss_progress_ += mean_square_error;
  if (frames_progress_ > progress_step) {
    ASLP_LOG << "ProgressLoss[last " << static_cast<int>(frames_progress_ / 100 / 3600) << "h of " << static_cast<int>(frames_ / 100 / 3600)
             << "h]: " << loss_progress_ / frames_progress_ << " (Mse)";
    loss_vec_.push_back(loss_progress_ / frames_progress_);
    frames_progress_ = 0;
    loss_progress_ = 0.0;
  }
}

// ASLP_MSE_FUSED=0: the reference's op sequence, its sum read in every minibatch
void Mse::EvalOps(const std::vector<BaseFloat> &frame_weights, const CuMatrixBase &net_out, const CuMatrixBase &target, CuMatrix *diff) {
  const int32 num_frames = MseNumFrames(frame_weights);
  HostVector hv;
  hv.data = frame_weights;
  frame_weights_ = hv;
  *diff = net_out;
  diff->AddMat(-1.0, target);
  diff->MulRowsVec(frame_weights_);
  CuMatrix diff_pow_2;
  diff_pow_2 = *diff;
  diff_pow_2.MulElements(diff_pow_2);
  diff_pow_2.MulRowsVec(frame_weights_);
  num_tgt_ = diff_pow_2.NumCols();
  AddBatch(0.5 * diff_pow_2.Sum(), num_frames);
}

double *Mse::PendingRoom(int32 rows) {
  static const int32 kMaxBatches = 32, kMaxRows = 1 << 16;
  if (rows != pending_rows_) {
    FlushPending();
    pending_rows_ = rows;
    pending_cap_ = std::max(1, std::min(kMaxBatches, kMaxRows / std::max(rows, 1)));
    // (zeroed: the double behind a batch's rows is read by the sum launch also where no kernel wrote it)
    if ((size_t)pending_.Dim() < (size_t)pending_cap_ * (rows + 1)) pending_.Resize(pending_cap_ * (rows + 1), kSetZero);
  }
  if (pending_batches_ == pending_cap_) FlushPending();
  return pending_.Data() + (size_t)(pending_batches_++) * (rows + 1);
}

static const int32 kMseMaxSums = 1024;   // {sum, frames} pairs the device holds between two fetches
void Mse::FlushPending() {
  if (pending_batches_ == 0) return;
  if (sums_.Dim() < 2 * kMseMaxSums) sums_.Resize(2 * kMseMaxSums, kSetZero);
  if (num_sums_ + pending_batches_ > kMseMaxSums) DrainSums();
  aslp_mse_batch_sums(pending_.Data(), pending_rows_, pending_batches_, sums_.Data() + 2 * (size_t)num_sums_);
  CheckK();
  num_sums_ += pending_batches_;
  pending_batches_ = 0;
}

// the summed batches into the host accumulators, in batch order: what the reference does once per minibatch
void Mse::DrainSums() {
  if (num_sums_ == 0) return;
  std::vector<double> h(2 * (size_t)num_sums_), frames(host_frames_.begin(), host_frames_.begin() + num_sums_);
  DeviceToHost(h.data(), sums_.Data(), sizeof(double) * h.size());
  host_frames_.erase(host_frames_.begin(), host_frames_.begin() + num_sums_);
  num_sums_ = 0;
  for (size_t b = 0; b < frames.size(); b++) AddBatch(0.5 * h[2 * b], frames[b] >= 0.0 ? frames[b] : h[2 * b + 1]);
}

void Mse::Fetch() {
  FlushPending();
  DrainSums();
  parked_frames_ = 0.0;
}

void Mse::EvalInto(const std::vector<BaseFloat> *frame_weights, const CuVectorBase *frame_weights_dev, const CuMatrixBase &net_out,
                   const CuMatrixBase &target, CuMatrixBase *diff, BaseFloat scale) {
  ASLP_ASSERT(net_out.NumCols() == target.NumCols() && net_out.NumRows() == target.NumRows());
  ASLP_ASSERT(net_out.NumCols() == diff->NumCols() && net_out.NumRows() == diff->NumRows());
  const int32 rows = net_out.NumRows();
  if (!Fused()) {
    std::vector<BaseFloat> w;
    if (frame_weights) {
      w = *frame_weights;
    } else {
      ASLP_ASSERT(frame_weights_dev != NULL && frame_weights_dev->Dim() == rows);
      w.resize(rows);
      frame_weights_dev->CopyToHost(w.data());
    }
    ASLP_ASSERT(rows == (int32)w.size());
    CuMatrix d;
    EvalOps(w, net_out, target, &d);
    if (scale != 1.0f) d.Scale(scale);
    diff->CopyFromMat(d);
    return;
  }
  double host_frames = -1.0;
  const float *w_dev;
  if (frame_weights) {
    ASLP_ASSERT(rows == (int32)frame_weights->size());
    host_frames = MseNumFrames(*frame_weights);
    HostVector hv;
    hv.data = *frame_weights;
    frame_weights_ = hv;
    w_dev = frame_weights_.Data();
  } else {
    ASLP_ASSERT(frame_weights_dev != NULL && frame_weights_dev->Dim() == rows);
    w_dev = frame_weights_dev->Data();
  }
  num_tgt_ = net_out.NumCols();
  // Is this the executor's loss diff (Nnet::LossDiff)?  No bound of |y - t| is known before the launch, so the kernel leaves the
  // per-workgroup maxima of |diff| with the layer that reads it: its conversion (PlaneHolder::Of) then skips the maximum pass.
  const S16DiffTarget t = s16_loss_diff_target();
  aslp_planes_out po = aslp_planes_out();
  PlaneSet *ps = nullptr;
  if (t.planes && t.diff == diff->Data()) {
    s16_loss_diff_target() = S16DiffTarget();
    if (t.planes->ReserveParts()) { ps = t.planes; po.parts = ps->Parts(); }
  }
  double *room = PendingRoom(rows);
  const int done = aslp_mse_eval_w(net_out.Data(), net_out.Dim(), target.Data(), target.Stride(), w_dev, scale, diff->Data(), diff->Stride(), room,
                                   ps ? &po : nullptr, frame_weights ? nullptr : room + rows);
  if (!done) pending_batches_--;
  CheckK();
  if (ps && po.nparts > 0) ps->TagParts(diff->Data(), po.nparts, t.epoch);
  host_frames_.push_back(host_frames);
  // progressive loss reporting (nnet-loss.cc:246-257) every 1h of frames: the threshold is known here, from the frames of the batches
  // fetched so far and of those parked since (their rows where only the device knows the count)
  static const int32 progress_step = 3600 * 100;
  parked_frames_ += host_frames >= 0.0 ? host_frames : rows;
  if (frames_progress_ + parked_frames_ > progress_step) Fetch();
}

void Mse::Eval(const std::vector<BaseFloat> &frame_weights, const CuMatrixBase &net_out, const CuMatrixBase &target, CuMatrix *diff) {
  // nnet-loss.cc:205-258
  ASLP_ASSERT(net_out.NumCols() == target.NumCols());
  ASLP_ASSERT(net_out.NumRows() == target.NumRows());
  ASLP_ASSERT(net_out.NumRows() == (int)frame_weights.size());
  if (!Fused()) { EvalOps(frame_weights, net_out, target, diff); return; }
  diff->Resize(net_out.NumRows(), net_out.NumCols(), kUndefined);
  EvalInto(&frame_weights, NULL, net_out, target, diff, 1.0f);
}
void Mse::EvalDevice(const CuVectorBase &frame_weights, const CuMatrixBase &net_out, const CuMatrixBase &target, CuMatrix *diff) {
  diff->Resize(net_out.NumRows(), net_out.NumCols(), kUndefined);
  EvalInto(NULL, &frame_weights, net_out, target, diff, 1.0f);
}
void Mse::Eval(const std::vector<BaseFloat> &frame_weights, const CuMatrixBase &net_out, const Posterior &post, CuMatrix *diff) {
  ASLP_ASSERT(net_out.NumRows() == (int32)post.size());
  PosteriorToMatrix(post, net_out.NumCols(), &tgt_mat_);
  Eval(frame_weights, net_out, tgt_mat_, diff);
}
std::string Mse::Report() {  // nnet-loss.cc:277-290
  Fetch();
  BaseFloat root_mean_square = sqrt(loss_ / frames_ / num_tgt_);
  std::ostringstream oss;
  oss << "AvgLoss: " << loss_ / frames_ << " (Mse), " << "[RMS " << root_mean_square << ", frames " << frames_ << "]" << std::endl;
  return oss.str();
}

void MultiTaskLoss::InitFromString(const std::string &s) {  // nnet-loss.cc:296-339
  std::vector<std::string> v;
  SplitStringToVector(s, ",:", false, &v);
  ASLP_ASSERT((v.size() - 1) % 3 == 0);
  ASLP_ASSERT(v[0] == "multitask");
  for (size_t i = 1; i < v.size(); i += 3) {
    if (v[i] == "xent") loss_vec_.push_back(new Xent());
    else if (v[i] == "mse") loss_vec_.push_back(new Mse());
    else ASLP_ERR << "Unknown objective function code : " << v[i];
    int32 dim;
    if (!ConvertStringToInteger(v[i + 1], &dim)) ASLP_ERR << "Cannot convert 'dim' " << v[i + 1] << " to integer!";
    loss_dim_.push_back(dim);
    BaseFloat weight;
    if (!ConvertStringToReal(v[i + 2], &weight)) ASLP_ERR << "Cannot convert 'weight' " << v[i + 2] << " to integer!";
    ASLP_ASSERT(weight >= 0.0);
    loss_weights_.push_back(weight);
  }
  loss_dim_offset_.assign(loss_dim_.size() + 1, 0);
  for (size_t i = 1; i <= loss_dim_.size(); i++) loss_dim_offset_[i] = loss_dim_offset_[i - 1] + loss_dim_[i - 1];
  ASLP_ASSERT(loss_vec_.size() > 0);
}
void MultiTaskLoss::Eval(const std::vector<BaseFloat> &fw, const CuMatrixBase &net_out, const Posterior &post, CuMatrix *diff) {
  int32 num_frames = net_out.NumRows(), num_output = net_out.NumCols();  // nnet-loss.cc:341-368
  ASLP_ASSERT(num_frames == (int32)post.size());
  ASLP_ASSERT(num_output == loss_dim_offset_.back());
  PosteriorToMatrix(post, num_output, &tgt_mat_);
  diff->Resize(num_frames, num_output);
  EvalTasks(fw, net_out, diff);
}
void MultiTaskLoss::EvalTasks(const std::vector<BaseFloat> &fw, const CuMatrixBase &net_out, CuMatrixBase *diff) {
  const int32 num_frames = net_out.NumRows();
  CuMatrix diff_aux;
  for (size_t i = 0; i < loss_vec_.size(); i++) {
    Mse *mse = Mse::Fused() ? dynamic_cast<Mse *>(loss_vec_[i]) : nullptr;
    if (mse) {   // straight into the task's column window, the task weight as the kernel's second rounding: no diff_aux, Scale, CopyFromMat
      ASLP_ASSERT(num_frames == (int32)fw.size());
      CuSubMatrix window = diff->ColRange(loss_dim_offset_[i], loss_dim_[i]);
      mse->EvalInto(&fw, NULL, net_out.ColRange(loss_dim_offset_[i], loss_dim_[i]), tgt_mat_.ColRange(loss_dim_offset_[i], loss_dim_[i]), &window,
                    loss_weights_[i]);
      continue;
    }
    loss_vec_[i]->Eval(fw, net_out.ColRange(loss_dim_offset_[i], loss_dim_[i]), tgt_mat_.ColRange(loss_dim_offset_[i], loss_dim_[i]), &diff_aux);
    diff_aux.Scale(loss_weights_[i]);
    diff->ColRange(loss_dim_offset_[i], loss_dim_[i]).CopyFromMat(diff_aux);
  }
}
static int g_multitask_fused = -1;   // -1: not asked yet (the environment decides)
bool MultiTaskLoss::Fused() {
  if (g_multitask_fused < 0) {
    const char *e = getenv("ASLP_MULTITASK_FUSED");
    g_multitask_fused = (e != nullptr && e[0] == '0') ? 0 : 1;
  }
  return g_multitask_fused != 0;
}
void MultiTaskLoss::SetFused(bool on) { g_multitask_fused = on ? 1 : 0; }

int32 MultiTaskLoss::NumXentTasks() const {
  int32 n = 0;
  for (int32 i = 0; i < NumTasks(); i++) n += Kind(i) == kXentTask ? 1 : 0;
  return n;
}
MultiTaskLoss::TaskKind MultiTaskLoss::Kind(int32 task) const { return dynamic_cast<const Xent *>(loss_vec_[task]) ? kXentTask : kMseTask; }
void MultiTaskLoss::GetTaskStats(int32 task, double out[5]) {
  ASLP_ASSERT(task >= 0 && task < NumTasks());
  for (int k = 0; k < 5; k++) out[k] = 0.0;
  if (Xent *x = dynamic_cast<Xent *>(loss_vec_[task])) x->GetStats(out);
  else dynamic_cast<Mse *>(loss_vec_[task])->GetStats(out);
}

void Xent::AddRowStats(const double *rowstats, int32 rows) {
  FlushPending();   // (the accumulators take the batches in evaluation order)
  aslp_xent_sum_rowstats(rowstats, rows, 1, stats_.Data());
}

void MultiTaskLoss::EvalDevice(const CuVectorBase &fw, const CuMatrixBase &in, bool pre_block_softmax, const int32 *labels_dev,
                               const CuMatrixBase *dense_targets, CuMatrixBase *diff) {
  const int32 rows = in.NumRows(), cols = in.NumCols(), num_tasks = NumTasks(), num_xent = NumXentTasks();
  ASLP_ASSERT(rows > 0 && cols == TotalDim() && fw.Dim() == rows);
  ASLP_ASSERT(diff != NULL && diff->NumRows() == rows && diff->NumCols() == cols);
  if (num_xent > 0 && labels_dev == NULL) ASLP_ERR << "MultiTaskLoss: an xent task needs labels";
  if (num_xent < num_tasks && (dense_targets == NULL || dense_targets->NumRows() != rows || dense_targets->NumCols() != cols))
    ASLP_ERR << "MultiTaskLoss: an mse task needs dense targets [" << rows << " x " << cols << "]";
  if (pre_block_softmax && (num_xent < num_tasks || !Fused())) ASLP_ERR << "MultiTaskLoss: only xent tasks on the fused route take a BlockSoftmax' input";
  // (the executor's offer to leave the diff's planes or maxima is for a loss that writes the whole diff: not taken, and not left for a
  //  task that writes a window of it)
  s16_loss_diff_target() = S16DiffTarget();
  if (!Fused()) {
    // today's op sequence: the dense target matrix scattered from the labels, then the tasks one by one as in Eval(Posterior)
    std::vector<int32> labels((size_t)rows * num_xent);
    if (num_xent > 0) DeviceToHost(labels.data(), labels_dev, sizeof(int32) * labels.size());
    Posterior post(rows);
    for (int32 i = 0, x = 0; i < num_tasks; i++) {
      if (Kind(i) != kXentTask) continue;
      for (int32 t = 0; t < rows; t++) {
        const int32 l = labels[(size_t)t * num_xent + x];
        if (l >= 0 && l < loss_dim_[i]) post[t].push_back(std::make_pair(loss_dim_offset_[i] + l, 1.0f));
      }
      x++;
    }
    PosteriorToMatrix(post, cols, &tgt_mat_);
    for (int32 i = 0; i < num_tasks; i++)
      if (Kind(i) == kMseTask) tgt_mat_.ColRange(loss_dim_offset_[i], loss_dim_[i]).CopyFromMat(dense_targets->ColRange(loss_dim_offset_[i], loss_dim_[i]));
    std::vector<BaseFloat> w(rows);
    fw.CopyToHost(w.data());
    EvalTasks(w, in, diff);
    return;
  }
  for (int32 i = 0; i < num_tasks; i++)
    if (Kind(i) == kXentTask && !aslp_xent_blocks_supported(loss_dim_[i])) ASLP_ERR << "MultiTaskLoss: unsupported xent task width " << loss_dim_[i];
  if (num_xent > 16) ASLP_ERR << "MultiTaskLoss: more than 16 xent tasks";
  if (num_xent > 0) {
    std::vector<aslp_xent_block> blocks;
    std::vector<Xent *> xents;
    bool own_room = false;
    for (int32 i = 0; i < num_tasks; i++) {
      Xent *x = dynamic_cast<Xent *>(loss_vec_[i]);
      if (!x) continue;
      aslp_xent_block b = {loss_dim_offset_[i], loss_dim_[i], loss_weights_[i], x->DeferredRoom(rows)};
      if (!b.rowstats) own_room = true;
      blocks.push_back(b);
      xents.push_back(x);
    }
    if (own_room) {   // too many rows to defer: the statistics are summed right behind the launch
      if ((size_t)rowstats_tmp_.Dim() < (size_t)rows * 5 * blocks.size()) rowstats_tmp_.Resize(rows * 5 * (int32)blocks.size(), kUndefined);
      for (size_t k = 0; k < blocks.size(); k++) blocks[k].rowstats = rowstats_tmp_.Data() + k * (size_t)rows * 5;
    }
    aslp_xent_blocks_eval(in.Data(), in.Dim(), blocks.data(), (int)blocks.size(), labels_dev, fw.Data(), diff->Data(), diff->Stride(),
                          pre_block_softmax ? 1 : 0, pre_block_softmax ? 1 : 0, nullptr, 0, nullptr);
    CheckK();
    for (size_t k = 0; k < xents.size(); k++) {
      if (own_room) xents[k]->AddRowStats(blocks[k].rowstats, rows);
      xents[k]->EvalDone(rows);
    }
  }
  for (int32 i = 0; i < num_tasks; i++) {
    Mse *mse = dynamic_cast<Mse *>(loss_vec_[i]);
    if (!mse) continue;
    CuSubMatrix window = diff->ColRange(loss_dim_offset_[i], loss_dim_[i]);
    mse->EvalInto(NULL, &fw, in.ColRange(loss_dim_offset_[i], loss_dim_[i]), dense_targets->ColRange(loss_dim_offset_[i], loss_dim_[i]), &window,
                  loss_weights_[i]);
  }
}

std::string MultiTaskLoss::Report() {  // nnet-loss.cc:370-393
  BaseFloat overall_loss = AvgLoss();
  std::ostringstream oss;
  oss << "MultiTaskLoss, with " << loss_vec_.size() << " parallel loss functions." << std::endl;
  for (size_t i = 0; i < loss_vec_.size(); i++) oss << "Loss " << i + 1 << ", " << loss_vec_[i]->Report() << std::endl;
  // (the reference streams both vectors through nnet-utils.h:42-45: every element followed by one blank, no brackets)
  oss << "Loss (OVERALL), " << "AvgLoss: " << overall_loss << " (MultiTaskLoss), " << "weights ";
  for (BaseFloat w : loss_weights_) oss << w << " ";
  oss << ", values ";
  for (LossItf *l : loss_vec_) oss << l->AvgLoss() << " ";
  oss << std::endl;
  return oss.str();
}
BaseFloat MultiTaskLoss::AvgLoss() {  // nnet-loss.cc:395-406
  BaseFloat ans(0.0);
  for (size_t i = 0; i < loss_vec_.size(); i++) {
    BaseFloat val = loss_weights_[i] * loss_vec_[i]->AvgLoss();
    if (!std::isfinite(val)) {
      ASLP_WARN << "Loss " << i + 1 << ", has bad objective function value '" << val << "', using 0.0 instead.";
      val = 0.0;
    }
    ans += val;
  }
  return ans;
}

}  // namespace aslp
