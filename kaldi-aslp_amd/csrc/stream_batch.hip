// stream_batch.hip -- a multi-stream batch built on the device: destination row r of a [B*S x D] matrix belongs to stream r % S and
// receives row src_frame[r] of that stream's source matrix (an utterance's features, kept in device memory), or +0.0 where
// src_frame[r] is -1.  A copy of bit patterns: no arithmetic touches the values, so NaN payloads and -0.0 come through.
#include <atomic>

#include "aslp_kernels.h"
#include "common.h"

namespace aslp {
namespace {

// VEC: four columns per 16-byte access; the launcher has checked D, both strides and every base for it.
// A frame outside [0, rows) is never read: the host refuses such a plan before the launch, and the kernel writes zeros for it all the same.
template <bool VEC>
__global__ void __launch_bounds__(kBlock) gather_stream_rows_kernel(float *dst, int ldd, int rows, int S, int D, const aslp_stream_src *src,
                                                                    const int32_t *src_frame) {
  constexpr int W = VEC ? 4 : 1;
  const int cw = D / W;
  const long n = (long)rows * cw;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int r = (int)(i / cw), c = (int)(i - (long)r * cw) * W;
    const aslp_stream_src t = src[r % S];
    const int f = src_frame[r];
    const bool live = f >= 0 && f < t.rows;
    if (VEC) {
      const uint4 v = live ? *reinterpret_cast<const uint4 *>(t.base + (long)f * t.stride + c) : make_uint4(0u, 0u, 0u, 0u);
      *reinterpret_cast<uint4 *>(dst + (long)r * ldd + c) = v;
    } else {
      const uint32_t v = live ? *reinterpret_cast<const uint32_t *>(t.base + (long)f * t.stride + c) : 0u;
      *reinterpret_cast<uint32_t *>(dst + (long)r * ldd + c) = v;
    }
  }
}

std::atomic<int> g_batch_host_override{-1};   // aslp_stream_batch_on_host(): -1 = ASLP_STREAM_BATCH_HOST decides

}  // namespace
}  // namespace aslp

using namespace aslp;

extern "C" {

void aslp_stream_batch_on_host(int on) { g_batch_host_override.store(on < 0 ? -1 : (on != 0)); }
int aslp_stream_batch_on_host_get(void) {
  const int o = g_batch_host_override.load();
  if (o >= 0) return o;
  static const bool env = [] { const char *e = getenv("ASLP_STREAM_BATCH_HOST"); return e != nullptr && e[0] == '1' && e[1] == 0; }();
  return env ? 1 : 0;
}

int aslp_gather_stream_rows_path(const float *dst, int ldd, int S, int D, const aslp_stream_src *src_host) {
  if ((D & 3) || (ldd & 3) || !aligned16(dst)) return 0;
  for (int s = 0; s < S; s++) {
    if (src_host[s].rows <= 0) continue;   // never read
    if ((src_host[s].stride & 3) || !aligned16(src_host[s].base)) return 0;
  }
  return 1;
}

int aslp_gather_stream_rows(float *dst, int ldd, int B, int S, int D, const aslp_stream_src *src_host, const aslp_stream_src *src_dev,
                            const int32_t *src_frame_host, const int32_t *src_frame_dev) {
  if (B < 0 || S <= 0 || D < 0 || ldd < D || (long)B * S > 0x7fffffffL) { set_error("aslp_gather_stream_rows: bad shape"); return 1; }
  if (B == 0 || D == 0) return 0;
  if (!dst || !src_host || !src_dev || !src_frame_host || !src_frame_dev) { set_error("aslp_gather_stream_rows: null argument"); return 1; }
  const int rows = B * S;
  for (int s = 0; s < S; s++) {
    const aslp_stream_src &t = src_host[s];
    if (t.rows < 0 || (t.rows > 0 && (!t.base || t.stride < D))) {
      set_error("aslp_gather_stream_rows: bad source of stream " + std::to_string(s));
      return 1;
    }
  }
  for (int r = 0; r < rows; r++) {
    const int f = src_frame_host[r];
    if (f < -1 || f >= src_host[r % S].rows) {
      set_error("aslp_gather_stream_rows: row " + std::to_string(r) + " asks for frame " + std::to_string(f) + " of a stream with " +
                std::to_string(src_host[r % S].rows) + " rows");
      return 1;
    }
  }
  if (aslp_gather_stream_rows_path(dst, ldd, S, D, src_host))
    hipLaunchKernelGGL((gather_stream_rows_kernel<true>), dim3(grid_for((long)rows * (D / 4))), dim3(kBlock), 0, cur_stream(), dst, ldd, rows, S, D,
                       src_dev, src_frame_dev);
  else
    hipLaunchKernelGGL((gather_stream_rows_kernel<false>), dim3(grid_for((long)rows * D)), dim3(kBlock), 0, cur_stream(), dst, ldd, rows, S, D,
                       src_dev, src_frame_dev);
  check_launch("gather_stream_rows");
  return 0;
}

}  // extern "C"
