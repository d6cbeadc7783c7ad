// gru_fused.hip -- the GRU recurrence (GruStreams, nnet-gru-streams.h:238-430) as four launches per timestep.
//
// Inside a timestep the GRU has two products that depend on each other in each direction of time:
//   forward   zr(t) += h(t-1) W_zr_h^T  -> z, r = sigmoid, g = r .* h(t-1)   then   m(t) += g(t) W_m_g^T -> m = tanh, h(t)
//   backward  d_h(t) += DZR(t+1) W_zr_h -> d_h, d_m                           then   d_g(t) = d_m(t) W_m_g -> d_r, d_z
// The reference issues each as a skinny cuBLAS GEMM (M = S streams) plus several elementwise launches.  Here each product
// is fused with the gate arithmetic that consumes it: a workgroup owns a 32 x 32 tile (32 streams x 32 gate columns), its 4
// waves split K, operands come straight from global memory as 16-byte loads (both K-contiguous: the backward kernels read
// transposed copies of the two recurrent matrices, refreshed once per Backpropagate), partial tiles meet in LDS in wave
// order (deterministic), and the epilogue finishes every (stream, cell) of the tile.
// Each launch has two entry points that differ in the product alone: gru_step_* on v_mfma_f32_32x32x2_f32 (product_f32 of rnn_mfma.h) and,
// opt-in (aslp_gru_step_pieces; contract in include/aslp_kernels.h), gru_step_*_h<NP> on v_mfma_f32_32x32x16_f16 with operands as NP fp16
// pieces (product_h / product_t_h): same grid, same contiguous K slice per wave, same reduction in wave order.  What surrounds the product
// -- the thread's epilogue operands (a struct and its load) and the gate arithmetic with its stores (finish) -- is written once per launch
// for fwd2, bwd1 and bwd2; such a kernel is indices, load, product, barrier, finish.  fwd1 keeps its loops in both of its kernels (see
// gru_step_fwd1).
#include "aslp_kernels.h"
#include "common.h"
#include "rnn_mfma.h"

namespace aslp {
namespace {

constexpr int kBwd1Waves = 4;  // K = 2H; 8 waves (two rounds of loads instead of four) measured no faster

// The epilogue operands of a thread's (stream, cell) pairs are requested before the product so their latency hides under it.
// All loads of the pairs first, stores last: a store in between would fence the later loads behind it (possible aliasing), i.e. one more
// round of memory latency per pair.

// ---- fwd2: m(t) += g(t) W_m_g^T; m, h(t)
struct GruFwd2 { float hp[4], zz[4], xm[4]; };
__device__ __forceinline__ GruFwd2 gru_fwd2_load(const float *y, const float *yp, int ld, int S, int H, int s0, int c0) {
  GruFwd2 e;
#pragma unroll
  for (int p = 0; p < 4; p++) {
    const int idx = threadIdx.x + 256 * p, sl = idx >> 5, cc = idx & 31;
    const int s = min(s0 + sl, S - 1), c = min(c0 + cc, H - 1);
    e.hp[p] = yp[(long)s * ld + 4 * H + c]; e.zz[p] = y[(long)s * ld + c]; e.xm[p] = y[(long)s * ld + 2 * H + c];
  }
  return e;
}
__device__ __forceinline__ void gru_fwd2_finish(const GruFwd2 &e, const float (*red)[32 * kPad], float *y, int ld, int S, int H, int s0, int c0) {
#pragma unroll
  for (int p = 0; p < 4; p++) {
    const int idx = threadIdx.x + 256 * p, sl = idx >> 5, cc = idx & 31;
    const int s = s0 + sl, c = c0 + cc;
    if (s >= S || c >= H) continue;
    float *ys = y + (long)s * ld;
    const float m = tanh_ref(e.xm[p] + tile_sum(red, sl, cc));
    ys[2 * H + c] = m;
    ys[4 * H + c] = e.hp[p] - e.hp[p] * e.zz[p] + e.zz[p] * m;
  }
}

// ---- bwd1: d_h(t) += [d_z | d_r](t+1) W_zr_h (K = 2H, read as W_zr_h^T [H x 2H]); d_h, d_m (gru_bwd1's arithmetic)
constexpr int kBwd1NE = 1024 / (64 * kBwd1Waves);   // (stream, cell) pairs per thread
struct GruBwd1 { float dhn[kBwd1NE], dh[kBwd1NE], zn[kBwd1NE], dgn[kBwd1NE], rn[kBwd1NE], m[kBwd1NE], z[kBwd1NE]; };
__device__ __forceinline__ GruBwd1 gru_bwd1_load(const float *d, const float *dn, const float *y, const float *yn, int ld, int S, int H, int s0, int c0) {
  GruBwd1 e;
#pragma unroll
  for (int p = 0; p < kBwd1NE; p++) {
    const int idx = threadIdx.x + 64 * kBwd1Waves * p, sl = idx >> 5, cc = idx & 31;
    const long o = (long)min(s0 + sl, S - 1) * ld;
    const int c = min(c0 + cc, H - 1);
    e.dhn[p] = dn[o + 4 * H + c]; e.dh[p] = d[o + 4 * H + c]; e.zn[p] = yn[o + c]; e.dgn[p] = dn[o + 3 * H + c]; e.rn[p] = yn[o + H + c];
    e.m[p] = y[o + 2 * H + c]; e.z[p] = y[o + c];
  }
  return e;
}
__device__ __forceinline__ void gru_bwd1_finish(const GruBwd1 &e, const float (*red)[32 * kPad], float *d, int ld, int S, int H, int s0, int c0) {
#pragma unroll
  for (int p = 0; p < kBwd1NE; p++) {
    const int idx = threadIdx.x + 64 * kBwd1Waves * p, sl = idx >> 5, cc = idx & 31;
    const int s = s0 + sl, c = c0 + cc;
    if (s >= S || c >= H) continue;
    const long o = (long)s * ld;
    const float dh = e.dh[p] + tile_sum<kBwd1Waves>(red, sl, cc) + e.dhn[p] - e.dhn[p] * e.zn[p] + e.dgn[p] * e.rn[p];
    d[o + 4 * H + c] = dh;
    d[o + 2 * H + c] = dtanh(e.m[p], dh * e.z[p]);
  }
}

// ---- bwd2: d_g(t) = d_m(t) W_m_g (K = H, read as W_m_g^T [H x H]); d_r, d_z (gru_bwd2's arithmetic)
struct GruBwd2 { float hp[4], dh[4], r[4], z[4], m[4]; };
__device__ __forceinline__ GruBwd2 gru_bwd2_load(const float *d, const float *y, const float *yp, int ld, int S, int H, int s0, int c0) {
  GruBwd2 e;
#pragma unroll
  for (int p = 0; p < 4; p++) {
    const int idx = threadIdx.x + 256 * p, sl = idx >> 5, cc = idx & 31;
    const long o = (long)min(s0 + sl, S - 1) * ld;
    const int c = min(c0 + cc, H - 1);
    e.hp[p] = yp[o + 4 * H + c]; e.dh[p] = d[o + 4 * H + c]; e.r[p] = y[o + H + c]; e.z[p] = y[o + c]; e.m[p] = y[o + 2 * H + c];
  }
  return e;
}
__device__ __forceinline__ void gru_bwd2_finish(const GruBwd2 &e, const float (*red)[32 * kPad], float *d, int ld, int S, int H, int s0, int c0) {
#pragma unroll
  for (int p = 0; p < 4; p++) {
    const int idx = threadIdx.x + 256 * p, sl = idx >> 5, cc = idx & 31;
    const int s = s0 + sl, c = c0 + cc;
    if (s >= S || c >= H) continue;
    const long o = (long)s * ld;
    const float dg = tile_sum(red, sl, cc);
    d[o + 3 * H + c] = dg;
    d[o + H + c] = dsigm(e.r[p], dg * e.hp[p]);
    d[o + c] = dsigm(e.z[p], e.dh[p] * e.m[p] - e.dh[p] * e.hp[p]);
  }
}

// ---- the kernels on the fp32 instruction
// fwd1: zr(t) += h(t-1) W_zr_h^T; z, r, g.  Columns of the tile: n < 16 -> z of cell c0 + n, n >= 16 -> r of cell c0 + n - 16.
// Its operand loads and gate arithmetic are written out here and in gru_step_fwd1_h: as a load and a finish function the LDS addresses of
// the two sums came out one instruction longer in all three kernels, and with two pieces at S = 20 the forward recurrence then measured
// 18.89 us per timestep against 18.90 to 18.92 of the commit before (profiles/step_kernels_shared_text.txt): outside its range, so the
// launch keeps the text it had, the product of gru_step_fwd1 included.
__global__ void __launch_bounds__(256) gru_step_fwd1(float *__restrict__ y, const float *__restrict__ yp, const float *__restrict__ w_zr_h, int ldw,
                                                     int ld, int S, int H, int no_product) {
  __shared__ float red[4][32 * kPad];
  const int c0 = blockIdx.x * 16, s0 = blockIdx.y * 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31;
  float xz[2], xr[2], hp[2];
#pragma unroll
  for (int p = 0; p < 2; p++) {
    const int idx = threadIdx.x + 256 * p, sl = idx >> 4, cc = idx & 15;
    const int s = min(s0 + sl, S - 1), c = min(c0 + cc, H - 1);
    xz[p] = y[(long)s * ld + c]; xr[p] = y[(long)s * ld + H + c]; hp[p] = yp[(long)s * ld + 4 * H + c];
  }
  {
    const int gate = l31 >> 4, cell = min(c0 + (l31 & 15), H - 1), h = lane >> 5;
    const float *arow = yp + (long)min(s0 + l31, S - 1) * ld + 4 * H;  // h(t-1)
    const float *brow = w_zr_h + (long)(gate * H + cell) * ldw;
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int nch = (H + 7) / 8, per = (nch + 3) / 4;
    if (!no_product) mfma_k_slices(acc, arow, brow, H, wave * per, min(nch, (wave + 1) * per), h);
    store_tile(red[wave], acc, lane);
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < 2; p++) {
    const int idx = threadIdx.x + 256 * p, sl = idx >> 4, cc = idx & 15;
    const int s = s0 + sl, c = c0 + cc;
    if (s >= S || c >= H) continue;
    float *ys = y + (long)s * ld;
    const float z = sigmoid_ref(xz[p] + tile_sum(red, sl, cc)), r = sigmoid_ref(xr[p] + tile_sum(red, sl, 16 + cc));
    ys[c] = z;
    ys[H + c] = r;
    ys[3 * H + c] = r * hp[p];
  }
}

__global__ void __launch_bounds__(256) gru_step_fwd2(float *__restrict__ y, const float *__restrict__ yp, const float *__restrict__ w_m_g, int ldw,
                                                     int ld, int S, int H) {
  __shared__ float red[4][32 * kPad];
  const int c0 = blockIdx.x * 32, s0 = blockIdx.y * 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31;
  const GruFwd2 e = gru_fwd2_load(y, yp, ld, S, H, s0, c0);
  const float *arow = y + (long)min(s0 + l31, S - 1) * ld + 3 * H;  // g(t)
  product_f32(red[wave], arow, w_m_g + (long)min(c0 + l31, H - 1) * ldw, H, wave, 4, lane, true);
  __syncthreads();
  gru_fwd2_finish(e, red, y, ld, S, H, s0, c0);
}

__global__ void __launch_bounds__(64 * kBwd1Waves) gru_step_bwd1(float *__restrict__ d, const float *__restrict__ dn, const float *__restrict__ y,
                                                     const float *__restrict__ yn, const float *__restrict__ w_t, int ldwt, int ld, int S, int H,
                                                     int has_next) {
  __shared__ float red[kBwd1Waves][32 * kPad];
  const int c0 = blockIdx.x * 32, s0 = blockIdx.y * 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31;
  const GruBwd1 e = gru_bwd1_load(d, dn, y, yn, ld, S, H, s0, c0);
  const float *arow = dn + (long)min(s0 + l31, S - 1) * ld;  // [d_z | d_r](t+1)
  product_f32(red[wave], arow, w_t + (long)min(c0 + l31, H - 1) * ldwt, 2 * H, wave, kBwd1Waves, lane, has_next != 0);
  __syncthreads();
  gru_bwd1_finish(e, red, d, ld, S, H, s0, c0);
}

__global__ void __launch_bounds__(256) gru_step_bwd2(float *__restrict__ d, const float *__restrict__ y, const float *__restrict__ yp,
                                                     const float *__restrict__ w_t, int ldwt, int ld, int S, int H) {
  __shared__ float red[4][32 * kPad];
  const int c0 = blockIdx.x * 32, s0 = blockIdx.y * 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31;
  const GruBwd2 e = gru_bwd2_load(d, y, yp, ld, S, H, s0, c0);
  const float *arow = d + (long)min(s0 + l31, S - 1) * ld + 2 * H;  // d_m(t)
  product_f32(red[wave], arow, w_t + (long)min(c0 + l31, H - 1) * ldwt, H, wave, 4, lane, true);
  __syncthreads();
  gru_bwd2_finish(e, red, d, ld, S, H, s0, c0);
}

// ---- the kernels on fp16 pieces (aslp_gru_step_pieces)
// the weight planes of one launch: hi / lo rows of ldp halves, *slot the bits of the bound they are scaled by
struct GruPlanes { const h16 *hi, *lo; const unsigned *slot; int ldp; };

template <int NP>
__global__ void __launch_bounds__(256) gru_step_fwd1_h(float *__restrict__ y, const float *__restrict__ yp, GruPlanes w, int ld, int S, int H) {
  __shared__ float red[4][32 * kPad];
  const int c0 = blockIdx.x * 16, s0 = blockIdx.y * 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31;
  float xz[2], xr[2], hp[2];
#pragma unroll
  for (int p = 0; p < 2; p++) {
    const int idx = threadIdx.x + 256 * p, sl = idx >> 4, cc = idx & 15;
    const int s = min(s0 + sl, S - 1), c = min(c0 + cc, H - 1);
    xz[p] = y[(long)s * ld + c]; xr[p] = y[(long)s * ld + H + c]; hp[p] = yp[(long)s * ld + 4 * H + c];
  }
  const int gate = l31 >> 4, cell = min(c0 + (l31 & 15), H - 1);
  const float *arow = yp + (long)min(s0 + l31, S - 1) * ld + 4 * H;  // h(t-1)
  const long boff = (long)(gate * H + cell) * w.ldp;
  product_h<NP>(red[wave], arow, H, w.hi + boff, NP == 2 ? w.lo + boff : w.hi + boff, w.slot, wave, 4, lane, true);
  __syncthreads();
#pragma unroll
  for (int p = 0; p < 2; p++) {
    const int idx = threadIdx.x + 256 * p, sl = idx >> 4, cc = idx & 15;
    const int s = s0 + sl, c = c0 + cc;
    if (s >= S || c >= H) continue;
    float *ys = y + (long)s * ld;
    const float z = sigmoid_ref(xz[p] + tile_sum(red, sl, cc)), r = sigmoid_ref(xr[p] + tile_sum(red, sl, 16 + cc));
    ys[c] = z;
    ys[H + c] = r;
    ys[3 * H + c] = r * hp[p];
  }
}

template <int NP>
__global__ void __launch_bounds__(256) gru_step_fwd2_h(float *__restrict__ y, const float *__restrict__ yp, GruPlanes w, int ld, int S, int H) {
  __shared__ float red[4][32 * kPad];
  const int c0 = blockIdx.x * 32, s0 = blockIdx.y * 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31;
  const GruFwd2 e = gru_fwd2_load(y, yp, ld, S, H, s0, c0);
  const float *arow = y + (long)min(s0 + l31, S - 1) * ld + 3 * H;  // g(t)
  const long boff = (long)min(c0 + l31, H - 1) * w.ldp;
  product_h<NP>(red[wave], arow, H, w.hi + boff, NP == 2 ? w.lo + boff : w.hi + boff, w.slot, wave, 4, lane, true);
  __syncthreads();
  gru_fwd2_finish(e, red, y, ld, S, H, s0, c0);
}

// w: the planes of W_zr_h^T [H x 2H]
template <int NP>
__global__ void __launch_bounds__(64 * kBwd1Waves) gru_step_bwd1_h(float *__restrict__ d, const float *__restrict__ dn, const float *__restrict__ y,
                                                                   const float *__restrict__ yn, GruPlanes w, int ld, int S, int H, int has_next) {
  __shared__ float red[kBwd1Waves][32 * kPad];
  const int c0 = blockIdx.x * 32, s0 = blockIdx.y * 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31;
  const GruBwd1 e = gru_bwd1_load(d, dn, y, yn, ld, S, H, s0, c0);
  const float *drow = dn + (long)min(s0 + l31, S - 1) * ld;  // [d_z | d_r](t+1)
  const long woff = (long)min(c0 + l31, H - 1) * w.ldp;
  product_t_h<NP>(red[wave], drow, 2 * H, w.hi + woff, NP == 2 ? w.lo + woff : w.hi + woff, w.slot, wave, kBwd1Waves, lane, has_next != 0);
  __syncthreads();
  gru_bwd1_finish(e, red, d, ld, S, H, s0, c0);
}

// w: the planes of W_m_g^T [H x H]
template <int NP>
__global__ void __launch_bounds__(256) gru_step_bwd2_h(float *__restrict__ d, const float *__restrict__ y, const float *__restrict__ yp, GruPlanes w,
                                                       int ld, int S, int H) {
  __shared__ float red[4][32 * kPad];
  const int c0 = blockIdx.x * 32, s0 = blockIdx.y * 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31;
  const GruBwd2 e = gru_bwd2_load(d, y, yp, ld, S, H, s0, c0);
  const float *drow = d + (long)min(s0 + l31, S - 1) * ld + 2 * H;  // d_m(t)
  const long woff = (long)min(c0 + l31, H - 1) * w.ldp;
  product_t_h<NP>(red[wave], drow, H, w.hi + woff, NP == 2 ? w.lo + woff : w.hi + woff, w.slot, wave, 4, lane, true);
  __syncthreads();
  gru_bwd2_finish(e, red, d, ld, S, H, s0, c0);
}

bool gru_args_ok(const void *p0, const void *p1, const void *p2, int ld, int ldw, int H) {
  return H % 4 == 0 && ld % 4 == 0 && ldw % 4 == 0 && aligned16(p0) && aligned16(p1) && aligned16(p2);
}

GruPlanes gru_planes(const void *hi, const void *lo, const unsigned *slot, int ldp) {
  return GruPlanes{static_cast<const h16 *>(hi), static_cast<const h16 *>(lo), slot, ldp};
}

// fp16 pieces on this path: opt-in (aslp_gru_step_pieces / ASLP_GRU_STEP_PIECES); under the umbrella (aslp_fp16_operands) the default is one piece,
// which measured 9 us per timestep below the fp32 instruction at H = 1024
int g_gru_step_override = -1;   // -1 = the environment decides
int gru_step_pieces() {
  static const int env = [] {
    const char *e = getenv("ASLP_GRU_STEP_PIECES");
    return (e != nullptr && (e[0] == '0' || e[0] == '1' || e[0] == '2') && e[1] == 0) ? e[0] - '0' : -1;
  }();
  if (g_gru_step_override >= 0) return g_gru_step_override;
  if (env >= 0) return env;
  return fp16_operands_on() ? 1 : 0;
}
thread_local int t_gru_step_last_pieces = 0;   // aslp_gru_step_last_pieces()

}  // namespace
}  // namespace aslp

using namespace aslp;

extern "C" {

int aslp_gru_step_supported(int H) { return H % 4 == 0; }

void aslp_gru_step_forward(float *y_cur, const float *y_prev, const float *w_zr_h, int ld_zr, const float *w_m_g, int ld_mg, int ld, int S, int H) {
  t_gru_step_last_pieces = 0;
  if (S <= 0 || H <= 0) return;
  if (!gru_args_ok(y_cur, y_prev, w_zr_h, ld, ld_zr, H) || ld_mg % 4 != 0 || !aligned16(w_m_g)) { set_error("aslp_gru_step_forward: unaligned operands"); return; }
  const int sb = (S + 31) / 32;
  hipLaunchKernelGGL(gru_step_fwd1, dim3((H + 15) / 16, sb), dim3(256), 0, cur_stream(), y_cur, y_prev, w_zr_h, ld_zr, ld, S, H, 0);
  hipLaunchKernelGGL(gru_step_fwd2, dim3((H + 31) / 32, sb), dim3(256), 0, cur_stream(), y_cur, y_prev, w_m_g, ld_mg, ld, S, H);
  check_launch("gru_step_forward");
}

void aslp_gru_step_backward(float *d_cur, const float *d_next, const float *y_cur, const float *y_next, const float *y_prev, const float *w_zr_h_t,
                            int ld_zr_t, const float *w_m_g_t, int ld_mg_t, int ld, int S, int H, int has_next) {
  t_gru_step_last_pieces = 0;
  if (S <= 0 || H <= 0) return;
  if (!gru_args_ok(d_cur, d_next, w_zr_h_t, ld, ld_zr_t, H) || ld_mg_t % 4 != 0 || !aligned16(w_m_g_t)) { set_error("aslp_gru_step_backward: unaligned operands"); return; }
  const int sb = (S + 31) / 32;
  hipLaunchKernelGGL(gru_step_bwd1, dim3((H + 31) / 32, sb), dim3(64 * kBwd1Waves), 0, cur_stream(), d_cur, d_next, y_cur, y_next, w_zr_h_t, ld_zr_t, ld, S, H,
                     has_next);
  hipLaunchKernelGGL(gru_step_bwd2, dim3((H + 31) / 32, sb), dim3(256), 0, cur_stream(), d_cur, y_cur, y_prev, w_m_g_t, ld_mg_t, ld, S, H);
  check_launch("gru_step_backward");
}

void aslp_gru_step_pieces(int n) { g_gru_step_override = (n >= 0 && n <= 2) ? n : -1; }
int aslp_gru_step_pieces_get(void) { return gru_step_pieces(); }
int aslp_gru_step_last_pieces(void) { return t_gru_step_last_pieces; }

void aslp_gru_step_forward_h(float *y_cur, const float *y_prev, const float *w_zr_h, int ld_zr, const float *w_m_g, int ld_mg, int ld, int S, int H,
                             const aslp_gru_step_h *p) {
  const int np = gru_step_pieces();
  if (np == 0) { aslp_gru_step_forward(y_cur, y_prev, w_zr_h, ld_zr, w_m_g, ld_mg, ld, S, H); return; }
  if (S <= 0 || H <= 0) return;
  if (H % 4 != 0 || ld % 4 != 0 || !aligned16(y_cur) || !aligned16(y_prev)) { set_error("aslp_gru_step_forward_h: unaligned operands"); return; }
  if (!p || !planes_ok(p->zr_hi, p->zr_lo, p->zr_slot, p->ldp_zr, H, np) || !planes_ok(p->mg_hi, p->mg_lo, p->mg_slot, p->ldp_mg, H, np)) {
    set_error("aslp_gru_step_forward_h: bad planes (needs hi / lo / slot per matrix, 16-byte aligned, ldp a multiple of 8 and >= K rounded up to 16)");
    return;
  }
  t_gru_step_last_pieces = np;
  const GruPlanes zr = gru_planes(p->zr_hi, p->zr_lo, p->zr_slot, p->ldp_zr), mg = gru_planes(p->mg_hi, p->mg_lo, p->mg_slot, p->ldp_mg);
  const dim3 g1((H + 15) / 16, (S + 31) / 32), g2((H + 31) / 32, (S + 31) / 32);
  if (np == 1) {
    hipLaunchKernelGGL(gru_step_fwd1_h<1>, g1, dim3(256), 0, cur_stream(), y_cur, y_prev, zr, ld, S, H);
    hipLaunchKernelGGL(gru_step_fwd2_h<1>, g2, dim3(256), 0, cur_stream(), y_cur, y_prev, mg, ld, S, H);
  } else {
    hipLaunchKernelGGL(gru_step_fwd1_h<2>, g1, dim3(256), 0, cur_stream(), y_cur, y_prev, zr, ld, S, H);
    hipLaunchKernelGGL(gru_step_fwd2_h<2>, g2, dim3(256), 0, cur_stream(), y_cur, y_prev, mg, ld, S, H);
  }
  check_launch("gru_step_forward_h");
}

void aslp_gru_step_backward_h(float *d_cur, const float *d_next, const float *y_cur, const float *y_next, const float *y_prev, const float *w_zr_h_t,
                              int ld_zr_t, const float *w_m_g_t, int ld_mg_t, int ld, int S, int H, int has_next, const aslp_gru_step_h *p) {
  const int np = gru_step_pieces();
  if (np == 0) { aslp_gru_step_backward(d_cur, d_next, y_cur, y_next, y_prev, w_zr_h_t, ld_zr_t, w_m_g_t, ld_mg_t, ld, S, H, has_next); return; }
  if (S <= 0 || H <= 0) return;
  if (H % 4 != 0 || ld % 4 != 0 || !aligned16(d_cur) || !aligned16(d_next)) { set_error("aslp_gru_step_backward_h: unaligned operands"); return; }
  if (!p || !planes_ok(p->zr_hi, p->zr_lo, p->zr_slot, p->ldp_zr, 2 * H, np) || !planes_ok(p->mg_hi, p->mg_lo, p->mg_slot, p->ldp_mg, H, np)) {
    set_error("aslp_gru_step_backward_h: bad planes (needs hi / lo / slot per matrix, 16-byte aligned, ldp a multiple of 8 and >= K rounded up to 16)");
    return;
  }
  t_gru_step_last_pieces = np;
  const GruPlanes zr = gru_planes(p->zr_hi, p->zr_lo, p->zr_slot, p->ldp_zr), mg = gru_planes(p->mg_hi, p->mg_lo, p->mg_slot, p->ldp_mg);
  const dim3 grid((H + 31) / 32, (S + 31) / 32);
  if (np == 1) {
    hipLaunchKernelGGL(gru_step_bwd1_h<1>, grid, dim3(64 * kBwd1Waves), 0, cur_stream(), d_cur, d_next, y_cur, y_next, zr, ld, S, H, has_next);
    hipLaunchKernelGGL(gru_step_bwd2_h<1>, grid, dim3(256), 0, cur_stream(), d_cur, y_cur, y_prev, mg, ld, S, H);
  } else {
    hipLaunchKernelGGL(gru_step_bwd1_h<2>, grid, dim3(64 * kBwd1Waves), 0, cur_stream(), d_cur, d_next, y_cur, y_next, zr, ld, S, H, has_next);
    hipLaunchKernelGGL(gru_step_bwd2_h<2>, grid, dim3(256), 0, cur_stream(), d_cur, y_cur, y_prev, mg, ld, S, H);
  }
  check_launch("gru_step_backward_h");
}

}  // extern "C"
