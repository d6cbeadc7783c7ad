// ctc_errors.hip -- CTC token errors of a batch on the device: the best path of every utterance (argmax ids, repeats collapsed, blanks
// dropped) and its unit-cost Levenshtein distance to the reference labels (WarpCtc::ErrorRate, aslp-nnet/warp-ctc.cc:487-529;
// Ctc::ErrorRate / ErrorRateMSeq, ctc-loss.cc:346-424).  One workgroup per utterance behind aslp_find_row_max_id; no workgroup talks to
// another.  Only the distance is formed: no caller reads the insertion / deletion / substitution split, and the distance is unique.
#include <algorithm>
#include <atomic>
#include <vector>

#include "aslp_ctc.h"
#include "aslp_kernels.h"
#include "common.h"
#include "ctc_errors.h"
#include "scratch.h"

namespace aslp {
namespace {

constexpr int kErrHypLds = 2048;   // hypothesis tokens a workgroup keeps in LDS; a longer hypothesis is read back from the scratch slot
constexpr int kErrMaxRef = 1024;   // one thread per reference token: the longest reference label sequence served

// ids: argmax of row f * num_seq + s.  meta: {frames, label offset, label count} per utterance, then the flat labels.
// res: {errors, hypothesis length} per utterance.  hyp_glob (nullable): hyp_ld ints per utterance; given when the caller wants the
// hypotheses or when one could outgrow the LDS copy.
__global__ void __launch_bounds__(kErrMaxRef) ctc_token_errors_kernel(const int *__restrict__ ids, const int *__restrict__ meta, int num_seq,
                                                                      int *__restrict__ hyp_glob, int hyp_ld, int *__restrict__ res) {
  __shared__ int s_hyp[kErrHypLds];
  __shared__ int s_diag[2][kErrMaxRef + 1];
  __shared__ int s_wave_total[kErrMaxRef / 64];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
  const int T = meta[3 * s], R = meta[3 * s + 2];
  const int *ref = meta + 3 * num_seq + meta[3 * s + 1];
  int *hyp_g = hyp_glob != nullptr ? hyp_glob + (long)s * hyp_ld : nullptr;

  // ---- best path: frame f emits its id iff id != 0 and (f == 0 or id != id(f - 1)); emitted ids compacted in frame order ----
  int H = 0;
  for (int f0 = 0; f0 < T; f0 += blockDim.x) {
    const int f = f0 + tid;
    int id = 0;
    bool emit = false;
    if (f < T) {
      id = ids[(long)f * num_seq + s];
      emit = id != 0 && (f == 0 || id != ids[(long)(f - 1) * num_seq + s]);
    }
    const unsigned long long votes = __ballot(emit);
    if (lane == 0) s_wave_total[wave] = __popcll(votes);
    __syncthreads();
    int pos = H + __popcll(votes & ((1ull << lane) - 1ull)), total = 0;
    for (int w = 0; w < nwaves; w++) {
      const int c = s_wave_total[w];
      if (w < wave) pos += c;
      total += c;
    }
    if (emit) {
      if (pos < kErrHypLds) s_hyp[pos] = id;
      if (hyp_g != nullptr) hyp_g[pos] = id;   // pos < T <= hyp_ld
    }
    H += total;
    __syncthreads();   // the wave totals are rewritten by the next chunk; the hypothesis is read by everyone below
  }

  // ---- edit distance d[H][R], d[h][0] = h, d[0][r] = r, over anti-diagonals k = h + r ----
  if (R == 0 || H == 0) {   // the same for the whole workgroup
    if (tid == 0) { res[2 * s] = R == 0 ? H : R; res[2 * s + 1] = H; }
    return;
  }
  // Thread c - 1 owns reference position c and walks down its column: at diagonal k it forms d[h][c], h = k - c, from its own
  // d[h - 1][c] (register), its left neighbour's d[h][c - 1] (written at diagonal k - 1: the other LDS row) and d[h - 1][c - 1] (what it
  // read from that neighbour one diagonal ago: register).  One barrier per diagonal: diagonal k reads row (k - 1) & 1 and writes row k & 1.
  const bool from_lds = H <= kErrHypLds;
  const int c = tid + 1;
  const int my_ref = c <= R ? ref[tid] : 0;
  int up = c, diag = c - 1;   // d[0][c], d[0][c - 1]
  for (int k = 2; k <= H + R; k++) {
    const int h = k - c;
    if (c <= R && h >= 1 && h <= H) {
      const int tok = from_lds ? s_hyp[h - 1] : hyp_g[h - 1];
      const int left = c == 1 ? h : s_diag[(k - 1) & 1][c - 1];
      const int v = min(min(up, left) + 1, diag + (tok != my_ref ? 1 : 0));
      diag = left;
      up = v;
      s_diag[k & 1][c] = v;
    }
    __syncthreads();
  }
  if (c == R) { res[2 * s] = up; res[2 * s + 1] = H; }
}

std::atomic<int> g_errors_host_override{-1};   // aslp_ctc_errors_on_host(): -1 = ASLP_CTC_ERRORS_HOST decides
std::atomic<int> g_errors_last_path{0};

inline long round64(long n) { return (n + 63) / 64 * 64; }

bool served(int max_frames, int max_label_len) { return max_frames >= 0 && max_label_len >= 0 && max_label_len <= kErrMaxRef; }

// the host path of the synchronous form: the argmax ids come back and the host collapses and measures them (distance only)
int host_edit_distance(const int *ref, int R, const std::vector<int> &hyp) {
  std::vector<int> prev(R + 1), cur(R + 1);
  for (int r = 0; r <= R; r++) prev[r] = r;
  for (size_t h = 1; h <= hyp.size(); h++) {
    cur[0] = (int)h;
    for (int r = 1; r <= R; r++) cur[r] = std::min(std::min(prev[r], cur[r - 1]) + 1, prev[r - 1] + (hyp[h - 1] != ref[r - 1] ? 1 : 0));
    prev.swap(cur);
  }
  return prev[R];
}

}  // namespace

bool ctc_errors_host_path() {
  static const bool env = [] { const char *e = getenv("ASLP_CTC_ERRORS_HOST"); return e != nullptr && e[0] == '1' && e[1] == 0; }();
  const int o = g_errors_host_override.load();
  return o >= 0 ? o != 0 : env;
}
void ctc_errors_note_path(int device) { g_errors_last_path.store(device); }

CtcErrorsJob::~CtcErrorsJob() {
  if (pending_) (void)hipEventSynchronize(static_cast<hipEvent_t>(done_));
  if (done_ != nullptr) (void)hipEventDestroy(static_cast<hipEvent_t>(done_));
  if (h_stage_ != nullptr) (void)hipHostFree(h_stage_);
  if (h_res_ != nullptr) (void)hipHostFree(h_res_);
}

bool CtcErrorsJob::Reserve(int **blk, long *cap, long ints) {
  if (ints <= *cap) return true;
  if (*blk != nullptr) (void)hipHostFree(*blk);
  *blk = nullptr;
  *cap = 0;
  const long want = ints < 4096 ? 4096 : ints + ints / 2;
  void *p = nullptr;
  const hipError_t e = hipHostMalloc(&p, sizeof(int) * want, hipHostMallocDefault);
  if (e != hipSuccess) { set_error(std::string("ctc token errors: hipHostMalloc: ") + hipGetErrorString(e)); return false; }
  *blk = static_cast<int *>(p);
  *cap = want;
  return true;
}

bool CtcErrorsJob::Wait() {
  if (!pending_) return false;
  pending_ = false;
  const hipError_t e = hipEventSynchronize(static_cast<hipEvent_t>(done_));
  if (e != hipSuccess) { set_error(std::string("ctc token errors: wait: ") + hipGetErrorString(e)); return false; }
  return true;
}

bool CtcErrorsJob::Enqueue(const float *net_out, MatrixDim d, const int *frames, int num_seq, const int *flat_labels, const int *label_lengths,
                           bool want_hyps) {
  if (pending_) (void)Wait();   // an unread batch is dropped; its upload no longer reads the staging
  if (net_out == nullptr || label_lengths == nullptr || num_seq <= 0 || d.rows <= 0 || d.cols <= 0 || (frames == nullptr && num_seq != 1))
    return false;
  int max_frames = 0, max_ref = 0;
  long num_labels = 0;
  for (int s = 0; s < num_seq; s++) {
    const int T = frames != nullptr ? frames[s] : d.rows;
    if (T < 0 || label_lengths[s] < 0) return false;
    max_frames = std::max(max_frames, T);
    max_ref = std::max(max_ref, label_lengths[s]);
    num_labels += label_lengths[s];
  }
  if (!served(max_frames, max_ref) || (long)max_frames * num_seq > d.rows || (num_labels > 0 && flat_labels == nullptr)) return false;
  const int used_rows = max_frames * num_seq;   // rows beyond the longest utterance are never looked at
  if (max_frames == 0) max_frames = 1;   // keeps the blocks below non-empty; no row is read

  const bool hyp_scratch = want_hyps || max_frames > kErrHypLds;
  const long n_up = 3L * num_seq + num_labels, n_ids = (long)max_frames * num_seq, n_hyp = hyp_scratch ? n_ids : 0;
  const long n_res = 2L * num_seq + (want_hyps ? n_ids : 0);
  if (!Reserve(&h_stage_, &stage_cap_, n_up) || !Reserve(&h_res_, &res_cap_, n_res)) return false;
  if (done_ == nullptr) {
    hipEvent_t ev = nullptr;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { set_error("ctc token errors: cannot create an event"); return false; }
    done_ = ev;
  }
  int *dev = static_cast<int *>(scratch(kScratchCtcErrors, sizeof(int) * (round64(n_ids) + round64(n_up) + round64(2L * num_seq) + n_hyp)));
  if (dev == nullptr) return false;
  int *d_ids = dev, *d_meta = d_ids + round64(n_ids), *d_res = d_meta + round64(n_up), *d_hyp = hyp_scratch ? d_res + round64(2L * num_seq) : nullptr;

  long off = 0;
  for (int s = 0; s < num_seq; s++) {
    h_stage_[3 * s] = frames != nullptr ? frames[s] : d.rows;
    h_stage_[3 * s + 1] = (int)off;
    h_stage_[3 * s + 2] = label_lengths[s];
    off += label_lengths[s];
  }
  if (num_labels > 0) std::copy(flat_labels, flat_labels + num_labels, h_stage_ + 3L * num_seq);

  hipStream_t stream = cur_stream();
  MatrixDim used = d;
  used.rows = used_rows;
  aslp_find_row_max_id(net_out, used, d_ids);
  if (hipMemcpyAsync(d_meta, h_stage_, sizeof(int) * n_up, hipMemcpyHostToDevice, stream) != hipSuccess) {
    set_error("ctc token errors: label upload failed");
    return false;
  }
  const int threads = std::max(64, (int)round64(max_ref));   // <= kErrMaxRef: served() looked
  hipLaunchKernelGGL(ctc_token_errors_kernel, dim3(num_seq), dim3(threads), 0, stream, d_ids, d_meta, num_seq, d_hyp, max_frames, d_res);
  check_launch("ctc_token_errors");
  hipError_t e = hipMemcpyAsync(h_res_, d_res, sizeof(int) * 2 * num_seq, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess && want_hyps) e = hipMemcpyAsync(h_res_ + 2L * num_seq, d_hyp, sizeof(int) * n_ids, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipEventRecord(static_cast<hipEvent_t>(done_), stream);
  if (e != hipSuccess) {
    set_error(std::string("ctc token errors: result copy: ") + hipGetErrorString(e));
    (void)hipStreamSynchronize(stream);   // nothing of this batch may still read the staging
    return false;
  }
  num_seq_ = num_seq;
  hyp_ld_ = max_frames;
  pending_ = true;
  return true;
}

}  // namespace aslp

using namespace aslp;

extern "C" {

int aslp_ctc_token_errors_supported(int max_frames, int max_label_len) { return served(max_frames, max_label_len) ? 1 : 0; }
void aslp_ctc_errors_on_host(int on) { g_errors_host_override.store(on < 0 ? -1 : (on != 0)); }
int aslp_ctc_errors_on_host_get(void) { return ctc_errors_host_path() ? 1 : 0; }
int aslp_ctc_errors_last_path(void) { return g_errors_last_path.load(); }

int aslp_ctc_token_errors(const float *net_out, MatrixDim d, const int *frames, int num_seq, const int *flat_labels, const int *label_lengths,
                          int *errors, int *hyp_lens, int *hyps, int hyp_ld) {
  if (net_out == nullptr || label_lengths == nullptr || errors == nullptr || hyp_lens == nullptr || num_seq <= 0 || d.rows <= 0 || d.cols <= 0 ||
      (frames == nullptr && num_seq != 1) || (hyps != nullptr && hyp_ld < 0))
    return 1;
  long num_labels = 0;
  for (int s = 0; s < num_seq; s++) {
    const int T = frames != nullptr ? frames[s] : d.rows;
    if (T < 0 || label_lengths[s] < 0 || (long)T * num_seq > d.rows) return 1;
    num_labels += label_lengths[s];
  }
  if (num_labels > 0 && flat_labels == nullptr) return 1;

  if (!ctc_errors_host_path()) {
    // one job per host thread, never given back: the HIP runtime may be gone when thread_local destructors run
    static thread_local CtcErrorsJob *job = new CtcErrorsJob();
    if (job->Enqueue(net_out, d, frames, num_seq, flat_labels, label_lengths, hyps != nullptr)) {
      ctc_errors_note_path(1);
      if (!job->Wait()) return 2;
      for (int s = 0; s < num_seq; s++) {
        errors[s] = job->Errors(s);
        hyp_lens[s] = job->HypLen(s);
        if (hyps != nullptr) std::copy(job->Hyp(s), job->Hyp(s) + std::min(hyp_lens[s], hyp_ld), hyps + (long)s * hyp_ld);
      }
      return 0;
    }
    if (has_error()) return 2;
  }
  // host path, whole: today's argmax launch, blocking copy and host loop
  ctc_errors_note_path(0);
  int *d_ids = static_cast<int *>(scratch(kScratchCtcErrors, sizeof(int) * (size_t)d.rows));
  if (d_ids == nullptr) return 2;
  std::vector<int> ids(d.rows), hyp;
  aslp_find_row_max_id(net_out, d, d_ids);
  if (hipMemcpyAsync(ids.data(), d_ids, sizeof(int) * (size_t)d.rows, hipMemcpyDeviceToHost, cur_stream()) != hipSuccess ||
      hipStreamSynchronize(cur_stream()) != hipSuccess) {
    set_error("aslp_ctc_token_errors: argmax copy failed");
    return 2;
  }
  long off = 0;
  for (int s = 0; s < num_seq; s++) {
    const int T = frames != nullptr ? frames[s] : d.rows;
    hyp.clear();
    int prev = -1;
    for (int f = 0; f < T; f++) {
      const int id = ids[(size_t)f * num_seq + s];
      if ((f == 0 || id != prev) && id != 0) hyp.push_back(id);
      prev = id;
    }
    errors[s] = host_edit_distance(flat_labels + off, label_lengths[s], hyp);
    hyp_lens[s] = (int)hyp.size();
    if (hyps != nullptr) std::copy(hyp.begin(), hyp.begin() + std::min((int)hyp.size(), hyp_ld), hyps + (long)s * hyp_ld);
    off += label_lengths[s];
  }
  return 0;
}

}  // extern "C"
