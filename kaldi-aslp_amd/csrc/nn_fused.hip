// nn_fused.hip -- fused hot-path ops: BatchNormalization forward/backward and Xent::Eval.
//
// Both are HBM-bound.  The reference issues ~25 elementwise /
// gemv launches per BatchNormalization step and ~15 + 5 blocking reductions per Xent::Eval;
// here BN forward is ONE column-statistics pass + 1 write pass (optionally producing the following Sigmoid's
// output as well), BN backward 1 statistics pass + 1 write pass (optionally absorbing that Sigmoid's backward), and Xent one pass with the row held in registers.
//
// The BatchNormalization kernels (three-launch, panel, cooperative, from-column-statistics) are built from one set of parts, each formula
// written once: bn_fwd_accum / bn_fwd_sums, bn_fwd_finalize, bn_fwd_out4 + bn_fwd_act4 / bn_fwd_write (forward); bn_bwd_load_rows, bn_bwd_fold,
// bn_bwd_accum / bn_bwd_sums, bn_bwd_col_update, bn_bwd_dvar_dmean, bn_bwd_coeffs, bn_bwd_write (backward); BnSlots (which rows and columns
// a thread holds) and wg_max.  The host picks the path in bn_path_for (which aslp_bn_path reports) and the instantiation in with_slots.
#include <atomic>
#include <type_traits>

#include "aslp_kernels.h"
#include "colreduce.h"
#include "common.h"
#include "split16.h"

namespace aslp {
unsigned *new_async_error_word(const char *what);  // runtime.cpp
namespace {

// Row r of a matrix as a float4 at column c, zero for rows at / past `end`.  The read itself is unconditional (clamped to the last valid
// row) and the zero a select on the VALUE: `r < end ? *p : zero` compiles to a pointer select against a zero kept in scratch memory and a
// flat load -- every kernel that spelled it that way carried a private segment.
__device__ __forceinline__ float4 load4_rows(const float *base, long ld, int r, int end, int c) {
  const int rc = r < end ? r : (end > 0 ? end - 1 : 0);
  float4 v = *reinterpret_cast<const float4 *>(base + (long)rc * ld + c);
  if (r >= end) v = make_float4(0.f, 0.f, 0.f, 0.f);
  return v;
}

// ---- BatchNormalization ---------------------------------------------------------------
// the ONE statistics pass: sum x and sum fl(x*x) in double for the running statistics
// (nnet-batch-normalization.h:216-220: the square is formed in float first), plus sum x*x with the
// product exact in double, from which the batch variance follows without a second pass over `in`:
//   var = E[x^2] - mean^2  evaluated in double (53-bit sums of 24-bit data: no cancellation problem),
// where the reference makes a second fp32 pass sum (x - mean)^2 (:193-204); the two agree to fp32
// rounding of the reference's own result, far inside the 1e-4 parity tolerance.
template <int VW>
__device__ __forceinline__ void bn_fwd_accum(const float (&v)[VW], double (&acc)[3][VW]) {
#pragma unroll
  for (int i = 0; i < VW; i++) {
    acc[0][i] += (double)v[i];
    acc[1][i] += (double)(v[i] * v[i]);
    acc[2][i] += (double)v[i] * (double)v[i];
  }
}
struct BnSum1F {
  static constexpr bool kVec = true;
  const float *in; int ld;
  template <int VW>
  __device__ void operator()(int r, int c, double (&acc)[3][VW]) const {
    float x[VW];
    loadv<VW>(in + (long)r * ld + c, x);
    bn_fwd_accum<VW>(x, acc);
  }
};
// The batch variance from the double sums, with `rows` itself as the divisor.  The fp32 1 / rows that scales the mean (as the reference's
// gemv does) is off by up to 2^-24 relative where rows is no power of two, and E[x^2] - mean^2 magnifies that by mean^2 / var: 6e-4 of the
// variance of a column at mean 100 with unit deviation, a "variance" of 6e-7 -- six floors -- for a column of one value 3.25.
__device__ __forceinline__ double bn_batch_var(double s0, double s2, int rows) {
  const double m = s0 / (double)rows;
  const double var = s2 / (double)rows - m * m;
  return var > 0.0 ? var : 0.0;
}
// One column's batch mean and inv_std from its three sums; `publish`: this thread also stores them and adds to the running sums (one
// workgroup per column does).
struct BnStat { float mu, is; };
__device__ __forceinline__ BnStat bn_fwd_finalize(double s0, double s1, double s2, int rows, float inv_rows, float floor_, bool publish, int col,
                                                  float *mean, float *inv_std, double *acc_means, double *acc_vars) {
  // the reference's mean is an fp32 gemv result scaled by 1/B; a double sum rounded once to
  // fp32 differs from it by < 1 ulp-of-sum.
  const float mu = (float)s0 * inv_rows;
  const double var = bn_batch_var(s0, s2, rows);
  const float is = 1.0f / sqrtf((float)var + floor_);
  if (publish) {
    mean[col] = mu;
    inv_std[col] = is;
    if (acc_means) acc_means[col] += s0;
    if (acc_vars) acc_vars[col] += s1;
  }
  return BnStat{mu, is};
}
struct BnSum1G {
  float inv_rows, floor_; int rows; float *mean, *inv_std; double *acc_means, *acc_vars;
  __device__ void operator()(int c, const double (&s)[3]) const {
    bn_fwd_finalize(s[0], s[1], s[2], rows, inv_rows, floor_, true, c, mean, inv_std, acc_means, acc_vars);
  }
};
// write pass: xhat = (x - mean) * inv_std ; out = xhat * gamma + beta ; optionally act = sigmoid(out) for a Sigmoid
// component fused behind the normalisation (then `out` itself may be NULL: nobody else reads it).  Four columns of row r at column c:
// bn_fwd_out4 returns `out`, bn_fwd_act4 the Sigmoid's output it stores, bn_fwd_write4 is the two.
__device__ __forceinline__ float4 bn_fwd_out4(const float4 &x, const float4 &m, const float4 &is, const float4 &g, const float4 &b, int r, int c,
                                              float *out, int ldo, float *xhat, int ldx) {
  float4 h, o;
  h.x = (x.x - m.x) * is.x; h.y = (x.y - m.y) * is.y; h.z = (x.z - m.z) * is.z; h.w = (x.w - m.w) * is.w;
  o.x = h.x * g.x + b.x; o.y = h.y * g.y + b.y; o.z = h.z * g.z + b.z; o.w = h.w * g.w + b.w;
  if (xhat) *reinterpret_cast<float4 *>(xhat + (long)r * ldx + c) = h;
  if (out) *reinterpret_cast<float4 *>(out + (long)r * ldo + c) = o;
  return o;
}
__device__ __forceinline__ float4 bn_fwd_act4(const float4 &o, int r, int c, float *act, int lda) {
  float4 y;
  y.x = sigmoid_ref(o.x); y.y = sigmoid_ref(o.y); y.z = sigmoid_ref(o.z); y.w = sigmoid_ref(o.w);
  *reinterpret_cast<float4 *>(act + (long)r * lda + c) = y;
  return y;
}
__device__ __forceinline__ void bn_fwd_write4(const float4 &x, const float4 &m, const float4 &is, const float4 &g, const float4 &b, int r, int c,
                                              float *out, int ldo, float *xhat, int ldx, float *act, int lda) {
  const float4 o = bn_fwd_out4(x, m, is, g, b, r, c, out, ldo, xhat, ldx);
  if (act) bn_fwd_act4(o, r, c, act, lda);
}
template <bool VEC>
__global__ void __launch_bounds__(kBlock) bn_normalize_kernel(const float *in, int ldi, float *out, int ldo, float *xhat, int ldx,
                                                              const float *mean, const float *inv_std, const float *scale,
                                                              const float *shift, int rows, int cols, float *act, int lda) {
  constexpr int W = VEC ? 4 : 1;
  int cw = cols / W;
  long n = (long)rows * cw;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    int r = (int)(i / cw), c = (int)(i - (long)r * cw) * W;
    if (VEC) {
      float4 x = *reinterpret_cast<const float4 *>(in + (long)r * ldi + c);
      float4 m = *reinterpret_cast<const float4 *>(mean + c), s = *reinterpret_cast<const float4 *>(inv_std + c);
      float4 g = *reinterpret_cast<const float4 *>(scale + c), b = *reinterpret_cast<const float4 *>(shift + c);
      bn_fwd_write4(x, m, s, g, b, r, c, out, ldo, xhat, ldx, act, lda);
    } else {
      float h = (in[(long)r * ldi + c] - mean[c]) * inv_std[c];
      if (xhat) xhat[(long)r * ldx + c] = h;
      const float o = h * scale[c] + shift[c];
      if (out) out[(long)r * ldo + c] = o;
      if (act) act[(long)r * lda + c] = sigmoid_ref(o);
    }
  }
}

// backward statistics: S1 = sum dy, S2 = sum xhat*dy
// `y` != NULL: a Sigmoid is fused behind the normalisation and `dy` is the diff w.r.t. ITS output;
// the diff w.r.t. the BN output is dy * y * (1 - y), formed on the fly (nnet-activation.h:170-173)
template <int VW>
__device__ __forceinline__ void bn_bwd_accum(const float (&d)[VW], const float (&h)[VW], float (&acc)[2][VW]) {
#pragma unroll
  for (int i = 0; i < VW; i++) {
    acc[0][i] += d[i];
    acc[1][i] += h[i] * d[i];
  }
}
struct BnBwdF {
  static constexpr bool kVec = true;
  const float *dy; int ldd; const float *xhat; int ldx; const float *y; int ldy;
  template <int VW>
  __device__ void operator()(int r, int c, float (&acc)[2][VW]) const {
    float d[VW], h[VW];
    loadv<VW>(dy + (long)r * ldd + c, d);
    loadv<VW>(xhat + (long)r * ldx + c, h);
    if (y) {
      float yy[VW];
      loadv<VW>(y + (long)r * ldy + c, yy);
#pragma unroll
      for (int i = 0; i < VW; i++) d[i] = d[i] * yy[i] * (1.0f - yy[i]);
    }
    bn_bwd_accum<VW>(d, h, acc);
  }
};
// One column's gradients from its sums S1, S2 and the values the column had before (g: the scale the forward pass used).
// `step`: the component's SGD step (nnet-batch-normalization.h:280-284) is taken right here instead of in a launch of
// its own; the write pass that follows still needs the scale the forward pass used, so the callers keep it.
__device__ __forceinline__ void bn_bwd_col_update(float s1, float s2, float mmt, float dshift_old, float dscale_old, float g, float shift_old, float neg_lr,
                                                  bool step, int col, float *dscale, float *dshift, float *scale, float *shift) {
  const float dsh = s1 + mmt * dshift_old, dsc = s2 + mmt * dscale_old;
  dshift[col] = dsh;
  dscale[col] = dsc;
  if (step) {
    scale[col] = g + neg_lr * dsc;
    shift[col] = shift_old + neg_lr * dsh;
  }
}
struct BnBwdG {
  float mmt; float *dscale, *dshift; float *s1, *s2;
  float *scale, *shift, *scale_used; float neg_lr; bool step;
  __device__ void operator()(int c, const float (&s)[2]) const {
    const float g = scale[c];
    bn_bwd_col_update(s[0], s[1], mmt, dshift[c], dscale[c], g, step ? shift[c] : 0.f, neg_lr, step, c, dscale, dshift, scale, shift);
    s1[c] = s[0];
    s2[c] = s[1];
    scale_used[c] = g;
  }
};
// the two per-column derivatives of the in_diff below
__device__ __forceinline__ void bn_bwd_dvar_dmean(float inv, float g, float s1, float s2, float &dvar, float &dmean) {
  dvar = -0.5f * inv * inv * g * s2;         // = sum (x-mean) D * (-0.5 inv^3)
  dmean = -inv * g * s1;
}
// in_diff: with D = dy*gamma, the reference's 4 steps (:238-276) reduce to
//   dvar  = -0.5 * inv^3 * sum (x-mean) * D      = -0.5 * inv^2 * gamma * S2
//   dmean = -inv * gamma * S1  ( - (2/B) dvar * sum(x-mean), which is 0 up to rounding )
//   in_diff = D*inv + (x-mean) * (2/B) * dvar + dmean/B,   (x-mean) = xhat/inv
template <bool VEC>
__global__ void __launch_bounds__(kBlock) bn_backward_kernel(const float *dy, int ldd, float *xhat, int ldx, const float *scale,
                                                             const float *inv_std, const float *s1, const float *s2, float *in_diff,
                                                             int ldi, int rows, int cols, const float *y, int ldy) {
  constexpr int W = VEC ? 4 : 1;
  int cw = cols / W;
  long n = (long)rows * cw;
  const float invB = 1.0f / (float)rows;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    int r = (int)(i / cw), c = (int)(i - (long)r * cw) * W;
    float dyv[W], hv[W], gv[W], iv[W], s1v[W], s2v[W], Dv[W], ov[W];
    if (VEC) {
      *reinterpret_cast<float4 *>(dyv) = *reinterpret_cast<const float4 *>(dy + (long)r * ldd + c);
      *reinterpret_cast<float4 *>(hv) = *reinterpret_cast<const float4 *>(xhat + (long)r * ldx + c);
      *reinterpret_cast<float4 *>(gv) = *reinterpret_cast<const float4 *>(scale + c);
      *reinterpret_cast<float4 *>(iv) = *reinterpret_cast<const float4 *>(inv_std + c);
      *reinterpret_cast<float4 *>(s1v) = *reinterpret_cast<const float4 *>(s1 + c);
      *reinterpret_cast<float4 *>(s2v) = *reinterpret_cast<const float4 *>(s2 + c);
    } else {
      dyv[0] = dy[(long)r * ldd + c]; hv[0] = xhat[(long)r * ldx + c]; gv[0] = scale[c]; iv[0] = inv_std[c];
      s1v[0] = s1[c]; s2v[0] = s2[c];
    }
    if (y) {
      float yv[W];
      if (VEC) *reinterpret_cast<float4 *>(yv) = *reinterpret_cast<const float4 *>(y + (long)r * ldy + c);
      else yv[0] = y[(long)r * ldy + c];
#pragma unroll
      for (int k = 0; k < W; k++) dyv[k] = dyv[k] * yv[k] * (1.0f - yv[k]);
    }
#pragma unroll
    for (int k = 0; k < W; k++) {
      float g = gv[k], inv = iv[k];
      float D = dyv[k] * g;
      float dvar, dmean;
      bn_bwd_dvar_dmean(inv, g, s1v[k], s2v[k], dvar, dmean);
      float xm = hv[k] / inv;
      Dv[k] = D;  // XsharpO_ <- dy*gamma, like the reference (:241-242)
      ov[k] = D * inv + xm * (2.0f * invB) * dvar + invB * dmean;
    }
    if (VEC) {
      *reinterpret_cast<float4 *>(xhat + (long)r * ldx + c) = *reinterpret_cast<float4 *>(Dv);
      *reinterpret_cast<float4 *>(in_diff + (long)r * ldi + c) = *reinterpret_cast<float4 *>(ov);
    } else {
      xhat[(long)r * ldx + c] = Dv[0];
      in_diff[(long)r * ldi + c] = ov[0];
    }
  }
}

// ---- BatchNormalization, panel-resident variants -----------------------------------------------------------------
// For minibatch-sized inputs (rows <= SLOTS * row lanes) a workgroup owns a panel of 4*CG columns over ALL rows and
// keeps it in registers: statistics, their finalize and the write pass are one launch that reads its operands once, instead
// of statistics stage 1 + stage 2 + write pass (3 launches, operands read twice).  These passes are latency-bound at
// [1024 x 2048] (8 MB, largely still in L2 / MALL behind the GEMM that produced it), so launches are what counts; each thread
// holds SLOTS rows of one 4-column group.
// Thread layout: column group fastest (CG adjacent threads read 16*CG contiguous bytes of a row), kPanelThreads / CG row
// lanes; a column's partial sums meet by wave shuffles, then across the waves in LDS, always in the same order.
constexpr int kPanelThreads = 256;
constexpr int kPanelWaves = kPanelThreads / kWave;

template <typename T, int N, int CG>
__device__ __forceinline__ void panel_reduce(T (&acc)[N][4], T *red /* [4 waves][CG][N*4] */) {
#pragma unroll
  for (int off = CG; off < kWave; off <<= 1)
#pragma unroll
    for (int a = 0; a < N; a++)
#pragma unroll
      for (int i = 0; i < 4; i++) acc[a][i] += __shfl_xor(acc[a][i], off);
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  if (lane < CG)
#pragma unroll
    for (int a = 0; a < N; a++)
#pragma unroll
      for (int i = 0; i < 4; i++) red[(wave * CG + lane) * (N * 4) + a * 4 + i] = acc[a][i];
  __syncthreads();
}
// after panel_reduce: total of accumulator a for panel column pc (0 .. 4*CG-1)
template <typename T, int N, int CG>
__device__ __forceinline__ T panel_total(const T *red, int a, int pc) {
  const int cg = pc / 4, i = pc % 4;
  T s = red[(0 * CG + cg) * (N * 4) + a * 4 + i];
#pragma unroll
  for (int w = 1; w < kPanelWaves; w++) s += red[(w * CG + cg) * (N * 4) + a * 4 + i];
  return s;
}
// The largest of one value per thread, in every thread of the workgroup.  red: kPanelWaves floats of LDS nobody else is using (a caller that
// has just read them puts a barrier in front).
__device__ __forceinline__ float wg_max(float v, float *red) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = red[0];
  for (int w = 1; w < kPanelWaves; w++) v = fmaxf(v, red[w]);
  return v;
}

// ---- the parts the panel-resident kernels are built from ---------------------------------------------------------------------------
// Which rows and columns a thread holds: workgroup q of the Q that share column panel p takes rows r0 .. r1 - 1 (a chunk of ceil(rows / Q)),
// a thread of it row(k) for slot k at the four columns from c.  The single-workgroup panels are Q = 1, q = 0, p = blockIdx.x.
// The parts take it BY VALUE: taken by reference every kernel built from them came out 1-3 % longer (a row's address formed from scratch
// per slot instead of base + c once; profiles/bn_parts_text.txt).
template <int CG>
struct BnSlots {
  static constexpr int L = kPanelThreads / CG;
  int r0, r1, cg, lane, c;
  __device__ __forceinline__ BnSlots(int rows, int Q, int q, int p) {
    const int rp = (rows + Q - 1) / Q;
    r0 = q * rp;
    r1 = min(rows, r0 + rp);
    cg = threadIdx.x % CG;
    lane = threadIdx.x / CG;
    c = (p * CG + cg) * 4;
  }
  __device__ __forceinline__ int row(int k) const { return r0 + lane + k * L; }
};
template <int SLOTS, int CG>
__device__ __forceinline__ void bn_load_slots(BnSlots<CG> s, const float *base, int ld, float4 (&x)[SLOTS]) {
#pragma unroll
  for (int k = 0; k < SLOTS; k++) x[k] = load4_rows(base, ld, s.row(k), s.r1, s.c);
}
template <int SLOTS>
__device__ __forceinline__ void bn_fwd_sums(const float4 (&x)[SLOTS], double (&acc)[3][4]) {
#pragma unroll
  for (int k = 0; k < SLOTS; k++) {
    const float v[4] = {x[k].x, x[k].y, x[k].z, x[k].w};
    bn_fwd_accum<4>(v, acc);
  }
}
template <int SLOTS, int CG>
__device__ __forceinline__ void bn_fwd_write(BnSlots<CG> s, const float4 (&x)[SLOTS], const float4 &m, const float4 &is, const float4 &g,
                                             const float4 &b, float *out, int ldo, float *xhat, int ldx, float *act, int lda) {
#pragma unroll
  for (int k = 0; k < SLOTS; k++) {
    const int r = s.row(k);
    if (r >= s.r1) break;
    bn_fwd_write4(x[k], m, is, g, b, r, s.c, out, ldo, xhat, ldx, act, lda);
  }
}
// dy into d[], and into h[] x_hat as the forward pass stored it or (RECOMPUTE) the layer input it is formed from again in bn_bwd_fold
template <int SLOTS, bool RECOMPUTE, int CG>
__device__ __forceinline__ void bn_bwd_load_rows(BnSlots<CG> s, const float *dy, int ldd, const float *xhat, int ldx, const float *xin, int ldxin,
                                                 float4 (&d)[SLOTS], float4 (&h)[SLOTS]) {
#pragma unroll
  for (int k = 0; k < SLOTS; k++) {
    const int r = s.row(k);
    d[k] = load4_rows(dy, ldd, r, s.r1, s.c);
    if (RECOMPUTE) h[k] = load4_rows(xin, ldxin, r, s.r1, s.c);
    else h[k] = load4_rows(xhat, ldx, r, s.r1, s.c);
  }
}
// RECOMPUTE: h[] <- (x - mean) * inv_std with the forward kernel's own two operations (same bits; m, is: the panel's batch mean and inv_std).
// HAS_Y: d[] <- the diff w.r.t. the BN output, dy * y * (1 - y), for a Sigmoid fused behind the normalisation.
template <int SLOTS, bool HAS_Y, bool RECOMPUTE, int CG>
__device__ __forceinline__ void bn_bwd_fold(BnSlots<CG> s, const float4 &m, const float4 &is, const float *y, int ldy, float4 (&d)[SLOTS],
                                            float4 (&h)[SLOTS]) {
  if (RECOMPUTE) {
#pragma unroll
    for (int k = 0; k < SLOTS; k++) {
      if (s.row(k) < s.r1) { h[k].x = (h[k].x - m.x) * is.x; h[k].y = (h[k].y - m.y) * is.y; h[k].z = (h[k].z - m.z) * is.z; h[k].w = (h[k].w - m.w) * is.w; }
    }
  }
  if (HAS_Y) {
#pragma unroll
    for (int k = 0; k < SLOTS; k++) {
      const float4 yy = load4_rows(y, ldy, s.row(k), s.r1, s.c);
      {
        // products rounded on their own, never contracted into the sums below: the values a separate Sigmoid backward would
        // have stored, so the folded and the unfolded executor agree bit for bit (HIP's __fmul_rn is a plain multiply)
#pragma clang fp contract(off)
        d[k].x = d[k].x * yy.x * (1.0f - yy.x); d[k].y = d[k].y * yy.y * (1.0f - yy.y);
        d[k].z = d[k].z * yy.z * (1.0f - yy.z); d[k].w = d[k].w * yy.w * (1.0f - yy.w);
      }
    }
  }
}
template <int SLOTS>
__device__ __forceinline__ void bn_bwd_sums(const float4 (&d)[SLOTS], const float4 (&h)[SLOTS], float (&acc)[2][4]) {
#pragma unroll
  for (int k = 0; k < SLOTS; k++) {
    const float dv[4] = {d[k].x, d[k].y, d[k].z, d[k].w}, hv[4] = {h[k].x, h[k].y, h[k].z, h[k].w};
    bn_bwd_accum<4>(dv, hv, acc);
  }
}
// per column of a thread's four: in_diff = D*inv + xm * ca + cb (stat: S1, S2 and the scale the forward pass used, per panel column)
template <int CG>
__device__ __forceinline__ void bn_bwd_coeffs(const float (&stat)[3][4 * CG], int cg, const float (&iv)[4], float invB, float (&gv)[4], float (&ca)[4],
                                              float (&cb)[4]) {
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const float g = stat[2][cg * 4 + i];
    float dvar, dmean;
    bn_bwd_dvar_dmean(iv[i], g, stat[0][cg * 4 + i], stat[1][cg * 4 + i], dvar, dmean);
    gv[i] = g;
    ca[i] = (2.0f * invB) * dvar;
    cb[i] = invB * dmean;
  }
}
// The write pass of the backward kernels: in_diff, and D = dy * scale into xhat where the forward pass stored one (like the reference,
// :241-242).  d[k] <- the in_diff written (for the planes), returns the largest |in_diff| of this thread.
template <int SLOTS, bool RECOMPUTE, int CG>
__device__ __forceinline__ float bn_bwd_write(BnSlots<CG> s, float4 (&d)[SLOTS], const float4 (&h)[SLOTS], const float (&gv)[4], const float (&iv)[4],
                                              const float (&ca)[4], const float (&cb)[4], float *xhat, int ldx, float *in_diff, int ldi) {
  float omax = 0.f;
#pragma unroll
  for (int k = 0; k < SLOTS; k++) {
    const int r = s.row(k);
    if (r >= s.r1) break;
    const float dv[4] = {d[k].x, d[k].y, d[k].z, d[k].w}, hv[4] = {h[k].x, h[k].y, h[k].z, h[k].w};
    float Dv[4], ov[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const float D = dv[i] * gv[i];
      const float xm = hv[i] / iv[i];
      Dv[i] = D;
      ov[i] = D * iv[i] + xm * ca[i] + cb[i];
    }
    if (!RECOMPUTE) *reinterpret_cast<float4 *>(xhat + (long)r * ldx + s.c) = make_float4(Dv[0], Dv[1], Dv[2], Dv[3]);
    *reinterpret_cast<float4 *>(in_diff + (long)r * ldi + s.c) = make_float4(ov[0], ov[1], ov[2], ov[3]);
    omax = s16_absmax4(omax, make_float4(ov[0], ov[1], ov[2], ov[3]));
    d[k] = make_float4(ov[0], ov[1], ov[2], ov[3]);
  }
  return omax;
}

template <int CG, int SLOTS>
__global__ void __launch_bounds__(kPanelThreads) bn_forward_panel(const float *__restrict__ in, int ldi, float *__restrict__ out, int ldo,
                                                           float *__restrict__ xhat, int ldx, const float *__restrict__ scale,
                                                           const float *__restrict__ shift, float *__restrict__ mean,
                                                           float *__restrict__ inv_std, double *__restrict__ acc_means,
                                                           double *__restrict__ acc_vars, float inv_rows, float floor_, int rows,
                                                           float *__restrict__ act, int lda) {
  __shared__ double red[kPanelWaves * CG * 12];
  __shared__ float stat[2][4 * CG];
  const BnSlots<CG> s(rows, 1, 0, (int)blockIdx.x);
  float4 x[SLOTS];
  bn_load_slots<SLOTS>(s, in, ldi, x);
  const float4 g = *reinterpret_cast<const float4 *>(scale + s.c), b = *reinterpret_cast<const float4 *>(shift + s.c);   // (in the rows' round trip)
  double acc[3][4] = {};
  bn_fwd_sums<SLOTS>(x, acc);
  panel_reduce<double, 3, CG>(acc, red);
  if (threadIdx.x < 4 * CG) {
    const int pc = threadIdx.x, col = (int)blockIdx.x * CG * 4 + pc;
    const double s0 = panel_total<double, 3, CG>(red, 0, pc), s1 = panel_total<double, 3, CG>(red, 1, pc), s2 = panel_total<double, 3, CG>(red, 2, pc);
    const BnStat st = bn_fwd_finalize(s0, s1, s2, rows, inv_rows, floor_, true, col, mean, inv_std, acc_means, acc_vars);
    stat[0][pc] = st.mu;
    stat[1][pc] = st.is;
  }
  __syncthreads();
  const float4 m = *reinterpret_cast<const float4 *>(&stat[0][s.cg * 4]), is = *reinterpret_cast<const float4 *>(&stat[1][s.cg * 4]);
  bn_fwd_write<SLOTS>(s, x, m, is, g, b, out, ldo, xhat, ldx, act, lda);
}

// RECOMPUTE: no normalised copy of the input was kept by the forward pass; x_hat = (x - mean) * inv_std is formed again from
// the layer input with the forward kernel's own two operations (same bits), and the in-place D = dy * scale the reference
// leaves in that buffer is not written at all -- 8.4 MB less traffic each way at [1024 x 2048].
template <int CG, int SLOTS, bool HAS_Y, bool RECOMPUTE>
__global__ void __launch_bounds__(kPanelThreads) bn_backward_panel(const float *__restrict__ dy, int ldd, float *__restrict__ xhat, int ldx,
                                                            float *__restrict__ scale, float *__restrict__ shift,
                                                            const float *__restrict__ inv_std, float *__restrict__ dscale,
                                                            float *__restrict__ dshift, float mmt, float neg_lr, bool step,
                                                            float *__restrict__ in_diff, int ldi, int rows, const float *__restrict__ y, int ldy,
                                                            const float *__restrict__ xin, int ldxin, const float *__restrict__ mean) {
  __shared__ float red[kPanelWaves * CG * 8];
  __shared__ float stat[3][4 * CG];  // S1, S2, the scale the forward pass used
  const BnSlots<CG> s(rows, 1, 0, (int)blockIdx.x);
  float4 d[SLOTS], h[SLOTS];
  bn_bwd_load_rows<SLOTS, RECOMPUTE>(s, dy, ldd, xhat, ldx, xin, ldxin, d, h);
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 m = RECOMPUTE ? *reinterpret_cast<const float4 *>(mean + s.c) : zero4, is = RECOMPUTE ? *reinterpret_cast<const float4 *>(inv_std + s.c) : zero4;
  bn_bwd_fold<SLOTS, HAS_Y, RECOMPUTE>(s, m, is, y, ldy, d, h);
  float acc[2][4] = {};
  bn_bwd_sums<SLOTS>(d, h, acc);
  panel_reduce<float, 2, CG>(acc, red);
  if (threadIdx.x < 4 * CG) {
    const int pc = threadIdx.x, col = (int)blockIdx.x * CG * 4 + pc;
    const float s1 = panel_total<float, 2, CG>(red, 0, pc), s2 = panel_total<float, 2, CG>(red, 1, pc);
    const float g = scale[col];
    bn_bwd_col_update(s1, s2, mmt, dshift[col], dscale[col], g, step ? shift[col] : 0.f, neg_lr, step, col, dscale, dshift, scale, shift);
    stat[0][pc] = s1;
    stat[1][pc] = s2;
    stat[2][pc] = g;
  }
  __syncthreads();
  if (in_diff == nullptr) return;
  const float4 iv4 = *reinterpret_cast<const float4 *>(inv_std + s.c);
  const float iv[4] = {iv4.x, iv4.y, iv4.z, iv4.w};
  float gv[4], ca[4], cb[4];
  bn_bwd_coeffs<CG>(stat, s.cg, iv, 1.0f / (float)rows, gv, ca, cb);
  bn_bwd_write<SLOTS, RECOMPUTE>(s, d, h, gv, iv, ca, cb, xhat, ldx, in_diff, ldi);
}

// ---- cooperative panels ---------------------------------------------------------------------------------------------
// The panel kernels above give a workgroup 16 columns over ALL rows: 128 workgroups for [1024 x 2048], half the chip idle and
// 64-byte row segments (measured 1.5-2.2 TB/s).  Here a column panel is 32 columns (one 128-byte line per row) and is shared
// by Q workgroups, each holding rows/Q rows in registers: 64 x 4 = 256 workgroups.  The Q partial statistics of a panel meet
// through a tiny inbox in global memory: every workgroup stores its partial into the inbox of each of the Q readers
// (agent-scope stores), every reader polls its own inbox until all Q partials are there, adds them in workgroup order
// (so all Q readers -- and every run -- get the same bits), and puts the "nothing here" pattern back before it leaves.
// The launch is ordered behind the previous one on its stream, so a reader-owned reset needs no further protocol.
// Workgroups p, p + P, p + 2P, ... share a panel: with P a multiple of 8 they sit on one XCD (speed only).
constexpr int kCoopCG = 8, kCoopCols = 32, kCoopLanes = kPanelThreads / kCoopCG;
constexpr unsigned long long kNothing = 0xFFFFFFFFFFFFFFFFull;
constexpr int kCoopSpinLimit = 1 << 22;  // polls before a reader gives up (seconds): the error word is raised, the output is garbage

template <int NW>  // 8-byte words per column
__device__ __forceinline__ bool coop_exchange(unsigned long long *inbox, int P, int Q, int p, int q, int pc, const unsigned long long (&mine)[NW],
                                              unsigned long long (*got)[NW] /* [Q][NW] */, unsigned *err) {
  // writer: my partial for column pc into every reader's inbox
  for (int qr = 0; qr < Q; qr++) {
    unsigned long long *dst = inbox + ((((size_t)p * Q + qr) * Q + q) * kCoopCols + pc) * NW;
#pragma unroll
    for (int w = 0; w < NW; w++) __hip_atomic_store(dst + w, mine[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // reader: all Q partials of column pc
  unsigned long long *src = inbox + (((size_t)p * Q + q) * Q * kCoopCols + pc) * NW;
  bool ok = true;
  for (int qw = 0; qw < Q; qw++) {
    unsigned long long *w0 = src + (size_t)qw * kCoopCols * NW;
    int spins = 0;
    for (;;) {
      bool all = true;
#pragma unroll
      for (int w = 0; w < NW; w++) { got[qw][w] = __hip_atomic_load(w0 + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); all &= got[qw][w] != kNothing; }
      if (all) break;
      if (++spins > kCoopSpinLimit) { ok = false; break; }
      __builtin_amdgcn_s_sleep(1);
    }
#pragma unroll
    for (int w = 0; w < NW; w++) __hip_atomic_store(w0 + w, kNothing, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // hand the slot back
  }
  if (!ok && pc == 0) __hip_atomic_fetch_add(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  return ok;
}

template <int SLOTS>
__global__ void __launch_bounds__(kPanelThreads) bn_forward_coop(const float *__restrict__ in, int ldi, float *__restrict__ out, int ldo,
                                                          float *__restrict__ xhat, int ldx, const float *__restrict__ scale,
                                                          const float *__restrict__ shift, float *__restrict__ mean,
                                                          float *__restrict__ inv_std, double *__restrict__ acc_means,
                                                          double *__restrict__ acc_vars, float inv_rows, float floor_, int rows,
                                                          float *__restrict__ act, int lda, int Q, unsigned long long *inbox, unsigned *err) {
  constexpr int CG = kCoopCG;
  __shared__ double red[kPanelWaves * CG * 12];
  __shared__ float stat[2][4 * CG];
  const int P = gridDim.x / Q, p = blockIdx.x % P, q = blockIdx.x / P;
  const BnSlots<CG> s(rows, Q, q, p);
  float4 x[SLOTS];
  bn_load_slots<SLOTS>(s, in, ldi, x);
  const float4 g = *reinterpret_cast<const float4 *>(scale + s.c), b = *reinterpret_cast<const float4 *>(shift + s.c);   // (in the rows' round trip)
  double acc[3][4] = {};
  bn_fwd_sums<SLOTS>(x, acc);
  panel_reduce<double, 3, CG>(acc, red);
  if (threadIdx.x < 4 * CG) {
    const int pc = threadIdx.x, col = p * CG * 4 + pc;
    unsigned long long mine[3], got[8][3];
#pragma unroll
    for (int a = 0; a < 3; a++) mine[a] = (unsigned long long)__double_as_longlong(panel_total<double, 3, CG>(red, a, pc));
    coop_exchange<3>(inbox, P, Q, p, q, pc, mine, got, err);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int qw = 0; qw < Q; qw++) {  // workgroup order: the same bits in all Q readers
      s0 += __longlong_as_double((long long)got[qw][0]);
      s1 += __longlong_as_double((long long)got[qw][1]);
      s2 += __longlong_as_double((long long)got[qw][2]);
    }
    const BnStat st = bn_fwd_finalize(s0, s1, s2, rows, inv_rows, floor_, q == 0, col, mean, inv_std, acc_means, acc_vars);
    stat[0][pc] = st.mu;
    stat[1][pc] = st.is;
  }
  __syncthreads();
  const float4 m = *reinterpret_cast<const float4 *>(&stat[0][s.cg * 4]), is = *reinterpret_cast<const float4 *>(&stat[1][s.cg * 4]);
  bn_fwd_write<SLOTS>(s, x, m, is, g, b, out, ldo, xhat, ldx, act, lda);
}

// BatchNormalization forward whose column statistics come from the producer of `in` (the forward GEMM's epilogue,
// aslp_gemm_epilogue.colstats: `groups` partial sums per column and statistic).  No statistics pass over the matrix, no exchange
// between workgroups: a workgroup adds the partials of its 32 columns (group order, double), then streams its rows once.
// Grid: (cols / 32) x Q row chunks like bn_forward_coop; every row chunk derives the same statistics, chunk 0 publishes them.
constexpr int kStatSlots = 4;
__global__ void __launch_bounds__(kPanelThreads) bn_forward_stats_kernel(const float *__restrict__ in, int ldi, float *__restrict__ out, int ldo,
                                                                        const float *__restrict__ scale, const float *__restrict__ shift,
                                                                        float *__restrict__ mean, float *__restrict__ inv_std,
                                                                        double *__restrict__ acc_means, double *__restrict__ acc_vars, float inv_rows,
                                                                        float floor_, int rows, float *__restrict__ act, int lda, int Q,
                                                                        const double *__restrict__ part, int groups, int ldp, S16Out po) {
  constexpr int CG = kCoopCG, COLS = kCoopCols, SL = kPanelThreads / COLS;  // SL partial-sum slices per column
  __shared__ double red[3][SL][COLS];
  __shared__ float stat[2][COLS];
  const int P = gridDim.x / Q, p = blockIdx.x % P, q = blockIdx.x / P;
  const BnSlots<CG> s(rows, Q, q, p);
  const int c = s.c;
  // the rows first (<= kStatSlots per thread, the host sizes Q for that): their latency overlaps the statistics below
  float4 x[kStatSlots];
  bn_load_slots<kStatSlots>(s, in, ldi, x);
  // everything else this workgroup reads goes out behind them in the same round: scale and shift, the planes' bound, and the statistics'
  // partial sums four groups at a time (a loop that adds one group per iteration is one round trip to L2 per iteration)
  const float4 g = *reinterpret_cast<const float4 *>(scale + c), b = *reinterpret_cast<const float4 *>(shift + c);
  const unsigned bound_bits = po.hi ? *po.slot : 0u;
  {
    const int pc = threadIdx.x % COLS, sl = threadIdx.x / COLS, col = p * COLS + pc;
    const long plane = (long)groups * ldp;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int g0 = sl; g0 < groups; g0 += 4 * SL) {
      double v[4][3];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int gi = g0 + u * SL;
        const double *pp = part + (long)(gi < groups ? gi : g0) * ldp + col;
        v[u][0] = pp[0]; v[u][1] = pp[plane]; v[u][2] = pp[2 * plane];
      }
#pragma unroll
      for (int u = 0; u < 4; u++)
        if (g0 + u * SL < groups) { s0 += v[u][0]; s1 += v[u][1]; s2 += v[u][2]; }   // (group order, as before)
    }
    red[0][sl][pc] = s0; red[1][sl][pc] = s1; red[2][sl][pc] = s2;
  }
  __syncthreads();
  if (threadIdx.x < COLS) {
    const int pc = threadIdx.x, col = p * COLS + pc;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int sl = 0; sl < SL; sl++) { s0 += red[0][sl][pc]; s1 += red[1][sl][pc]; s2 += red[2][sl][pc]; }
    const BnStat st = bn_fwd_finalize(s0, s1, s2, rows, inv_rows, floor_, q == 0, col, mean, inv_std, acc_means, acc_vars);   // as bn_forward_coop
    stat[0][pc] = st.mu;
    stat[1][pc] = st.is;
  }
  __syncthreads();
  const float4 m = *reinterpret_cast<const float4 *>(&stat[0][s.cg * 4]), is = *reinterpret_cast<const float4 *>(&stat[1][s.cg * 4]);
  const float pscale = po.hi ? ldexpf(1.f, s16_exponent(bound_bits)) : 0.f;
#pragma unroll
  for (int k = 0; k < kStatSlots; k++) {
    const int r = s.row(k);
    if (r >= s.r1) break;
    const float4 o = bn_fwd_out4(x[k], m, is, g, b, r, c, out, ldo, nullptr, 0);
    if (act) {
      const float4 y = bn_fwd_act4(o, r, c, act, lda);
      if (po.hi) {   // the planes of the activations for the products that read them (bound: a sigmoid's 1)
        half4 hi, lo;
        s16_split4(y, pscale, &hi, &lo);
        *reinterpret_cast<half4 *>(po.hi + (long)r * po.ld + c) = hi;
        *reinterpret_cast<half4 *>(po.lo + (long)r * po.ld + c) = lo;
      }
    }
  }
}

// The largest of one value per workgroup, in every workgroup of a launch whose workgroups are all resident at once (the host checks: they
// wait for each other).  They meet in gmax, one 8-byte word each: this launch's token | the value's bits -- nothing to reset, an older
// launch's word never matches.  mine: the workgroup's value (in every thread); red: >= kPanelWaves floats of LDS nobody else is using.
__device__ __forceinline__ float coop_grid_max(float mine, unsigned long long *gmax, unsigned token, unsigned *err, float *red) {
  if (threadIdx.x == 0)
    __hip_atomic_store(gmax + blockIdx.x, ((unsigned long long)token << 32) | (unsigned long long)__float_as_uint(mine), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  float gm = 0.f;
  bool ok = true;
  for (int i = threadIdx.x; i < (int)gridDim.x; i += kPanelThreads) {
    int spins = 0;
    for (;;) {
      const unsigned long long v = __hip_atomic_load(gmax + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((unsigned)(v >> 32) == token) { gm = fmaxf(gm, __uint_as_float((unsigned)v)); break; }
      if (++spins > kCoopSpinLimit) { ok = false; break; }
      __builtin_amdgcn_s_sleep(1);
    }
  }
  if (!ok) __hip_atomic_fetch_add(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __syncthreads();   // (a caller may have just read red[])
  return wg_max(gm, red);
}

// Matrices (up to kS16MaxJobs, blockIdx.y) copied (optional) and their fp16 planes made in ONE launch (coop_convert_launch: the network
// input -- copy + maximum pass + conversion pass were three launches in front of the first layer product -- and PlaneSet::ConvertFrom /
// ConvertMany): a thread holds U 16-byte pieces of its matrix, the workgroups of a matrix find its maximum among themselves as above.  A
// matrix whose bound is given (parts) takes it from there.
// RAGGED: a matrix of the launch has a width that is no multiple of 4 (the host chooses, under gemm_split16_ragged()): a row then has one
// more piece, the group that holds its last column -- loaded and copied column by column (split16.h s16_load4_ragged), its planes written
// whole, with zeros from column `cols` on (inside the planes' pitch, which is a multiple of 4: zeros belong there).
struct CoopConvJobs { CoopConvJob j[kS16MaxJobs]; };
template <int U, bool RAGGED = false>
__global__ void __launch_bounds__(kPanelThreads) copy_planes_coop(CoopConvJobs jobs, unsigned long long *gmax, unsigned token, unsigned *err, SeqFillJob fill) {
  __shared__ float red[kPanelWaves];
  if (fill.buf0 != nullptr) {   // (uniform) a recurrent layer's buffer preparation rides along: stores only, spread over the launch's workgroups
    const int per = (fill.T + 2) * fill.S, nb = (int)(gridDim.x * gridDim.y);
    for (int r = (int)(blockIdx.y * gridDim.x + blockIdx.x); r < 2 * per; r += nb) seq_fill_row(fill, r % per, r / per);
  }
  const CoopConvJob job = jobs.j[blockIdx.y];
  const int rows = job.pl.rows, cols = job.pl.cols, c4 = RAGGED ? (cols + 3) >> 2 : cols >> 2, units = rows * c4;
  float4 v[U];
  int rr[U], cc[U];
  float m = 0.f;
#pragma unroll
  for (int k = 0; k < U; k++) {
    const int u = ((int)blockIdx.x * U + k) * kPanelThreads + (int)threadIdx.x;
    const int r = u / c4;
    rr[k] = u < units ? r : -1;
    cc[k] = 4 * (u - r * c4);
    if constexpr (RAGGED) v[k] = u < units ? s16_load4_ragged(job.src + (long)r * job.ld_src, cc[k], cols) : make_float4(0.f, 0.f, 0.f, 0.f);
    else v[k] = u < units ? *reinterpret_cast<const float4 *>(job.src + (long)r * job.ld_src + cc[k]) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (job.parts != nullptr) {   // (uniform) the bound is known: every workgroup reads it
    for (int i0 = threadIdx.x; i0 < job.nparts; i0 += 4 * kPanelThreads) {
      float p[4];
#pragma unroll
      for (int q = 0; q < 4; q++) { const int i = i0 + q * kPanelThreads; p[q] = i < job.nparts ? job.parts[i] : 0.f; }
      m = fmaxf(fmaxf(m, fmaxf(p[0], p[1])), fmaxf(p[2], p[3]));
    }
  }
#pragma unroll
  for (int k = 0; k < U; k++) {
    if constexpr (RAGGED) {
      if (rr[k] >= 0 && job.dst != nullptr) {
        float *d = job.dst + (long)rr[k] * job.ld_dst + cc[k];
        if (cc[k] + 4 <= cols) {
          *reinterpret_cast<float4 *>(d) = v[k];
        } else {   // (the copy's row ends where the source's does: nothing is written behind it)
          d[0] = v[k].x;
          if (cc[k] + 1 < cols) d[1] = v[k].y;
          if (cc[k] + 2 < cols) d[2] = v[k].z;
        }
      }
    } else {
      if (rr[k] >= 0 && job.dst != nullptr) *reinterpret_cast<float4 *>(job.dst + (long)rr[k] * job.ld_dst + cc[k]) = v[k];
    }
    if (job.parts == nullptr) m = s16_absmax4(m, v[k]);
  }
  m = wg_max(m, red);
  unsigned mbits = __float_as_uint(m);
  if (job.parts == nullptr) mbits = __float_as_uint(coop_grid_max(m, gmax + (size_t)blockIdx.y * gridDim.x, token, err, red));
  if (blockIdx.x == 0 && threadIdx.x == 0) *job.pl.slot = mbits;
  const float ps = ldexpf(1.f, s16_exponent(mbits));
#pragma unroll
  for (int k = 0; k < U; k++) {
    if (rr[k] < 0) continue;
    half4 hi, lo;
    s16_split4(v[k], ps, &hi, &lo);
    *reinterpret_cast<half4 *>(job.pl.hi + (long)rr[k] * job.pl.ld + cc[k]) = hi;
    *reinterpret_cast<half4 *>(job.pl.lo + (long)rr[k] * job.pl.ld + cc[k]) = lo;
  }
}

// what bn_backward_coop needs to bound its in-diff before it has written it (see there)
template <int SLOTS, bool HAS_Y, bool RECOMPUTE>
__global__ void __launch_bounds__(kPanelThreads) bn_backward_coop(const float *__restrict__ dy, int ldd, float *__restrict__ xhat, int ldx,
                                                           float *__restrict__ scale, float *__restrict__ shift,
                                                           const float *__restrict__ inv_std, float *__restrict__ dscale,
                                                           float *__restrict__ dshift, float mmt, float neg_lr, bool step,
                                                           float *__restrict__ in_diff, int ldi, int rows, const float *__restrict__ y, int ldy,
                                                           const float *__restrict__ xin, int ldxin, const float *__restrict__ mean, int Q,
                                                           unsigned long long *inbox, unsigned *err, float *__restrict__ max_parts, S16Out po,
                                                           unsigned long long *gmax, unsigned token) {
  constexpr int CG = kCoopCG;
  __shared__ float red[kPanelWaves * CG * 8];
  __shared__ float stat[3][4 * CG];  // S1, S2, the scale the forward pass used
  const int P = gridDim.x / Q, p = blockIdx.x % P, q = blockIdx.x / P;
  const BnSlots<CG> s(rows, Q, q, p);
  const int c = s.c;
  float4 d[SLOTS], h[SLOTS];
  bn_bwd_load_rows<SLOTS, RECOMPUTE>(s, dy, ldd, xhat, ldx, xin, ldxin, d, h);
  // the per-column values go out in the rows' round trip (a load issued where its value is first used costs a trip to L2 of its own there).
  // The scale the forward pass used: workgroup q == 0 rewrites it (the folded SGD step) only after it has seen every partial of the panel,
  // and a workgroup publishes its partial only after this load has returned (the wait in front of the exchange).
  const float4 iv4 = *reinterpret_cast<const float4 *>(inv_std + c);
  const bool col_thread = threadIdx.x < 4 * CG;
  const int my_col = p * CG * 4 + (int)threadIdx.x;
  const float g_fwd = col_thread ? scale[my_col] : 0.f;
  const float dsh_old = col_thread && q == 0 ? dshift[my_col] : 0.f, dsc_old = col_thread && q == 0 ? dscale[my_col] : 0.f;
  const float sh_old = col_thread && q == 0 && step ? shift[my_col] : 0.f;
  const float4 m4 = RECOMPUTE ? *reinterpret_cast<const float4 *>(mean + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  bn_bwd_fold<SLOTS, HAS_Y, RECOMPUTE>(s, m4, iv4, y, ldy, d, h);
  float acc[2][4] = {};
  bn_bwd_sums<SLOTS>(d, h, acc);
  panel_reduce<float, 2, CG>(acc, red);
  if (threadIdx.x < 4 * CG) {
    const int pc = threadIdx.x, col = p * CG * 4 + pc;
    unsigned long long mine[1], got[8][1];
    const float p1 = panel_total<float, 2, CG>(red, 0, pc), p2 = panel_total<float, 2, CG>(red, 1, pc);
    mine[0] = ((unsigned long long)__float_as_uint(p2) << 32) | (unsigned long long)__float_as_uint(p1);   // one granule: {S2, S1}
    const float g = g_fwd;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (g_fwd has landed before the partial is published; see the top)
    coop_exchange<1>(inbox, P, Q, p, q, pc, mine, got, err);
    float s1 = 0.f, s2 = 0.f;
    for (int qw = 0; qw < Q; qw++) { s1 += __uint_as_float((unsigned)got[qw][0]); s2 += __uint_as_float((unsigned)(got[qw][0] >> 32)); }
    stat[0][pc] = s1;
    stat[1][pc] = s2;
    stat[2][pc] = g;
    if (q == 0) bn_bwd_col_update(s1, s2, mmt, dsh_old, dsc_old, g, sh_old, neg_lr, step, col, dscale, dshift, scale, shift);
  }
  __syncthreads();
  if (in_diff != nullptr) {
    const float iv[4] = {iv4.x, iv4.y, iv4.z, iv4.w};
    float gv[4], ca[4], cb[4];
    bn_bwd_coeffs<CG>(stat, s.cg, iv, 1.0f / (float)rows, gv, ca, cb);
    const float omax = bn_bwd_write<SLOTS, RECOMPUTE>(s, d, h, gv, iv, ca, cb, xhat, ldx, in_diff, ldi);   // (d[] <- in_diff, kept for the planes below)
    if (max_parts != nullptr || po.hi != nullptr) {   // this workgroup's largest |in_diff|
      __syncthreads();            // (red[] is free: every thread is past the statistics)
      const float m = wg_max(omax, red);
      // ... for the conversion of in_diff, which takes its scale from these (split16.h) ...
      if (max_parts != nullptr && threadIdx.x == 0) max_parts[blockIdx.x] = m;
      // ... or the planes from this launch: the workgroups' maxima meet (coop_grid_max) and every workgroup scales its rows by the matrix
      // maximum, exactly as the conversion pass would have.
      if (po.hi != nullptr) {
        const float gm = coop_grid_max(m, gmax, token, err, red);
        const unsigned mbits = __float_as_uint(gm);
        if (blockIdx.x == 0 && threadIdx.x == 0) *const_cast<unsigned *>(po.slot) = mbits;   // for the products (launched behind this kernel)
        const float ps = ldexpf(1.f, s16_exponent(mbits));
#pragma unroll
        for (int k = 0; k < SLOTS; k++) {
          const int r = s.row(k);
          if (r >= s.r1) break;
          half4 hi, lo;
          s16_split4(d[k], ps, &hi, &lo);
          *reinterpret_cast<half4 *>(po.hi + (long)r * po.ld + c) = hi;
          *reinterpret_cast<half4 *>(po.lo + (long)r * po.ld + c) = lo;
        }
      }
    }
  }
}
constexpr int kCoopGmaxWords = 1024;   // workgroups whose maxima may meet in one launch
// Host threads of this process that launch cooperative kernels.  With more than one, the launches that wait for ALL their workgroups are not
// used: two of them (or one beside another thread's persistent recurrence) half resident on one chip would wait for each other's
// unplaced workgroups -- the same reason as device_shared() (scratch.h), between threads instead of processes.
// (the count lives in runtime.cpp -- register_grid_wide_thread -- because the persistent recurrences' launchers register in it too: a thread
//  that only ever runs recurrences never comes through coop_state())
struct CoopState {
  unsigned long long *inbox = nullptr, *gmax = nullptr;
  unsigned *err = nullptr, token = 0;
  bool tried = false;
};
// (per host thread: launches of different threads run side by side on their own streams and must not meet in one exchange area)
CoopState &coop_state() {
  static thread_local CoopState st;
  if (!st.tried) {
    st.tried = true;
    register_grid_wide_thread();
    const size_t words = (size_t)256 * 8 * 8 * kCoopCols * 3;  // up to 256 panels x Q <= 8 readers x 8 writers
    unsigned long long *p = nullptr;
    if (hipMalloc(&p, words * 8) == hipSuccess && hipMemset(p, 0xFF, words * 8) == hipSuccess) {
      st.err = new_async_error_word("cooperative kernel (BatchNormalization / input planes): a workgroup timed out waiting for the other workgroups of its "
                                    "launch (results of that call are invalid; if several processes share this GPU set ASLP_DEVICE_SHARED=1)");
      if (st.err) st.inbox = p;
      unsigned long long *gm = nullptr;
      if (st.inbox && hipMalloc(&gm, kCoopGmaxWords * 8) == hipSuccess && hipMemset(gm, 0, kCoopGmaxWords * 8) == hipSuccess) st.gmax = gm;   // (token 0 is never used)
    }
  }
  return st;
}
// may a launch wait for every one of its workgroups?  (a device of this process' own, one launching host thread, the main stream)
inline bool coop_grid_wide_ok() { return !device_shared() && !on_side_stream() && grid_wide_threads() <= 1; }
inline int coop_cu_count() {
  static int num_cu = [] { hipDeviceProp_t pr; int d = 0; return (hipGetDevice(&d) == hipSuccess && hipGetDeviceProperties(&pr, d) == hipSuccess) ? pr.multiProcessorCount : 0; }();
  return num_cu;
}
// rows x cols served by the cooperative kernels?  returns Q (row parts per panel) and the slots per thread, or Q = 0
struct CoopShape { int q, slots; };
inline CoopShape bn_coop_shape(int rows, int cols) {
  static const int forced = [] { const char *e = getenv("ASLP_BN_COOP"); return e ? atoi(e) : -1; }();
  CoopShape none = {0, 0};
  if (forced == 0 || cols % kCoopCols != 0) return none;
  const int num_cu = coop_cu_count();
  const int P = cols / kCoopCols;
  if (P > 256 || num_cu <= 0) return none;
  int Q = num_cu / P;              // every workgroup resident at once, one per CU (they wait for each other)
  Q = Q > 4 ? 4 : Q;
  if (Q < 2) return none;
  const int rp = (rows + Q - 1) / Q;
  if (rp < 64) return none;        // small batches: the single-workgroup panels are already launch-latency bound
  for (int slots : {4, 8, 16})
    if (rp <= slots * kCoopLanes) return CoopShape{Q, slots};
  return none;
}

// 0: the three-launch path; else the row slots per thread (4, 8 or 16) of a panel of kPanelCG column groups per workgroup.  Measured on
// the cfg2 step (1024 x 2048): 4 groups x 256 threads 729 k frames/s, 2 groups (32-byte row segments) 698 k, 1024-thread workgroups with
// 4 / 8 groups 680 k / 713 k, the three-launch path 717-721 k.
constexpr int kPanelCG = 4;
inline int bn_panel_shape(int rows, int cols) {
  static const int forced = [] { const char *e = getenv("ASLP_BN_PANEL"); return e ? atoi(e) : -1; }();
  if (forced == 0 || cols % (4 * kPanelCG) != 0) return 0;
  for (int slots : {4, 8, 16})
    if (rows <= slots * (kPanelThreads / kPanelCG)) return slots;
  return 0;
}
// The kernels that serve [rows x cols]: 0 the three launches, 1 the single-workgroup panels, 2 the cooperative panels (q workgroups per
// panel); vec: every operand allows 16-byte accesses.  The launchers and aslp_bn_path both ask here.
struct BnPath { int path, q, slots; };
inline BnPath bn_path_for(int rows, int cols, bool vec) {
  const int slots = vec ? bn_panel_shape(rows, cols) : 0;
  if (!slots) return BnPath{0, 0, 0};
  const CoopShape cs = bn_coop_shape(rows, cols);
  if (cs.q && coop_state().inbox) return BnPath{2, cs.q, cs.slots};
  return BnPath{1, 1, slots};
}
// 16-byte accesses to rows of `stride` floats from p on (a vector: stride 0)
inline bool vec_ok(const void *p, int stride = 0) { return aligned16(p) && stride % 4 == 0; }
// f(std::integral_constant) for the slot count / the flag given at run time: the kernels' template arguments
template <typename F>
void with_slots(int slots, F &&f) {
  switch (slots) {
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
  }
}
template <typename F>
void with_flag(bool flag, F &&f) {
  if (flag) f(std::true_type{});
  else f(std::false_type{});
}

// ---- Xent ------------------------------------------------------------------------------
constexpr int kXentPerThread = 32;  // cols <= 8192 cached in registers

// stats[0..4] += {frames, correct, -xent, -entropy, likelihood} summed over the rows in a fixed order (thread t: rows t, t + 256, ...; the
// 64 lanes of a wave; the four waves), by one workgroup of 256 threads.  coherent: the rows were written by other workgroups of the SAME launch
// (device-scope loads; unused by the shipped callers).  Four rows' loads are in flight at a time.
template <bool RAW = false>   // RAW: the five sums as they are into stats[0..4] (xent_apply_kernel adds them to the accumulators later)
__device__ __forceinline__ void xent_sum_rows(const double *rowstats, int rows, double *stats, bool coherent) {
  __shared__ double sh_sum[4][5];
  double a[5] = {0, 0, 0, 0, 0};
  for (int r0 = threadIdx.x; r0 < rows; r0 += 4 * 256) {
    double v[4][5];
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
      for (int k = 0; k < 5; k++) {
        const int r = r0 + u * 256;
        const double *p = rowstats + (long)(r < rows ? r : r0) * 5 + k;
        const double x = coherent ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *p;
        v[u][k] = r < rows ? x : 0.0;
      }
#pragma unroll
    for (int u = 0; u < 4; u++)
      if (r0 + u * 256 < rows) {   // (adding the 0.0 of a missing row would turn a -0.0 sum into +0.0)
#pragma unroll
        for (int k = 0; k < 5; k++) a[k] += v[u][k];
      }
  }
#pragma unroll
  for (int k = 0; k < 5; k++) a[k] = wave_sum_d(a[k]);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < 5; k++) sh_sum[threadIdx.x >> 6][k] = a[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    double s[5];
    for (int k = 0; k < 5; k++) s[k] = sh_sum[0][k] + sh_sum[1][k] + sh_sum[2][k] + sh_sum[3][k];
    if (RAW) {
      for (int k = 0; k < 5; k++) stats[k] = s[k];
      return;
    }
    stats[0] += s[0];
    stats[1] += s[1];
    stats[2] += -s[2];
    stats[3] += -s[3];
    stats[4] += s[4];
  }
}

// One block (256 threads) per row.  rowstats[r][0..4] = {w, correct*w, w*sum t log(y+1e-20),
// w*sum t log(t+1e-20), w*sum t y} as double; summed in fixed order by xent_finalize.
// SOFTMAX: `y` holds the activations in front of the network's final Softmax and the row softmax is formed here,
// with exactly the arithmetic of softmax_rows_kernel<256> (same lane -> column mapping, same reduction order), so
// folding the Softmax component into the loss changes no bit; `y_out` (nullable) receives the posteriors.
// SPARSE (with DENSE): the targets come as CSR -- row r's entries are row_begin[r] .. row_begin[r + 1] - 1 of `labels` (the columns, strictly
// increasing within a row) and `t` (the weights); an entry whose column is outside [0, cols) is skipped and never used as an address.  The
// row's entries are laid out in LDS as the dense row they stand for (0.0f + w: what an add onto a zeroed matrix leaves, so -0.0 becomes +0.0),
// each thread fills its slots from there through its own column map, and everything behind that is the DENSE arithmetic as it stands: the
// same bits as the dense kernel on the dense matrix.  The lanes that laid an entry out write the zero back once the row has been read, so the
// staging row is cleared once per workgroup.
template <bool DENSE, bool SOFTMAX, int PER, bool VEC = false, bool SPARSE = false>
__global__ void __launch_bounds__(256) xent_rows_kernel(const float *y, int ldy, const float *t, int ldt, const int32_t *labels,
                                                        const float *fw, float *diff, int ldd, int rows, int cols, double *rowstats,
                                                        float *y_out, int ldyo, S16Out po, const int32_t *row_begin) {
  static_assert(!SPARSE || DENSE, "CSR targets are dense targets to the arithmetic");
  constexpr bool TMAT = DENSE && !SPARSE;   // the targets are read from a matrix
  __shared__ __attribute__((aligned(16))) float stage[SPARSE ? 256 * PER : 1];
  // VEC: slot k of a thread is column 4 (tid + 256 (k / 4)) + k % 4, every array touched 16 bytes at a time (softmax_rows_kernel's second
  // map, chosen by the same rule: cols % 4 == 0 and 16-byte aligned rows); else column tid + 256 k
  static_assert(!VEC || PER % 4 == 0, "whole groups of four slots");
  __shared__ float shf[4][4];
  __shared__ int shi[4][2];
  __shared__ float shs[4];
  const float pscale = po.hi ? ldexpf(1.f, s16_exponent(*po.slot)) : 0.f;   // planes of diff for the product that reads it (split16.h)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  auto col_of = [tid](int k) { return VEC ? 4 * (tid + (k >> 2) * 256) + (k & 3) : tid + k * 256; };
  if (SPARSE) {
#pragma unroll
    for (int k = 0; k < PER; k++) stage[tid + k * 256] = 0.0f;
    __syncthreads();
  }
  for (int r = blockIdx.x; r < rows; r += gridDim.x) {
    const float *yr = y + (long)r * ldy;
    const float *tr = TMAT ? t + (long)r * ldt : nullptr;
    const int label = DENSE ? -1 : labels[r];
    const float fw_r = fw[r];   // (here, in the row's round trip: read where it is used it is a trip of its own behind the last reduction)
    // SPARSE: the thread's first entry leaves in front of the row's loads (a row of more than 256 entries takes further rounds below)
    int e_end = 0, e_next = 0, e_col = -1;
    float e_w = 0.0f;
    if (SPARSE) {
      e_end = row_begin[r + 1];
      e_next = row_begin[r] + tid;
      if (e_next < e_end) { e_col = labels[e_next]; e_w = t[e_next]; }
      e_next += 256;
    }
    float yv[PER], tv[PER];
    float tsum = 0.0f, ybest = -1e21f, tbest = -1e21f;
    int yi = -1, ti = -1;
    // the row (activations or posteriors), as many loads in flight as the thread has slots
    if (VEC) {
#pragma unroll
      for (int k4 = 0; k4 < PER / 4; k4++) {
        const int c = 4 * (tid + k4 * 256);
        if (c < cols) {
          const float4 v4 = *reinterpret_cast<const float4 *>(yr + c);
          yv[4 * k4] = v4.x; yv[4 * k4 + 1] = v4.y; yv[4 * k4 + 2] = v4.z; yv[4 * k4 + 3] = v4.w;
          if (TMAT) {
            const float4 t4 = *reinterpret_cast<const float4 *>(tr + c);
            tv[4 * k4] = t4.x; tv[4 * k4 + 1] = t4.y; tv[4 * k4 + 2] = t4.z; tv[4 * k4 + 3] = t4.w;
          }
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < PER; k++) {
        const int c = tid + k * 256;
        if (c < cols) {
          yv[k] = yr[c];
          if (TMAT) tv[k] = tr[c];
        }
      }
    }
    if (SPARSE) {
      if (e_col >= 0 && e_col < cols) stage[e_col] = 0.0f + e_w;
      for (int i = e_next; i < e_end; i += 256) {
        const int c = labels[i];
        if (c >= 0 && c < cols) stage[c] = 0.0f + t[i];
      }
      __syncthreads();
      if (VEC) {
#pragma unroll
        for (int k4 = 0; k4 < PER / 4; k4++) {
          const int c = 4 * (tid + k4 * 256);
          if (c < cols) {
            const float4 t4 = *reinterpret_cast<const float4 *>(stage + c);
            tv[4 * k4] = t4.x; tv[4 * k4 + 1] = t4.y; tv[4 * k4 + 2] = t4.z; tv[4 * k4 + 3] = t4.w;
          }
        }
      } else {
#pragma unroll
        for (int k = 0; k < PER; k++) {
          const int c = tid + k * 256;
          if (c < cols) tv[k] = stage[c];
        }
      }
    }
    if (SOFTMAX) {
      float m = -INFINITY;
#pragma unroll
      for (int k = 0; k < PER; k++)
        if (col_of(k) < cols) m = fmaxf(m, yv[k]);
      m = wave_max(m);
      if (lane == 0) shs[w] = m;
      __syncthreads();
      m = fmaxf(fmaxf(fmaxf(shs[0], shs[1]), shs[2]), shs[3]);
      __syncthreads();
      float sum = 0.0f;
#pragma unroll
      for (int k = 0; k < PER; k++) {
        if (col_of(k) < cols) {
          yv[k] = expf(yv[k] - m);
          sum += yv[k];
        }
      }
      sum = wave_sum(sum);
      if (lane == 0) shs[w] = sum;
      __syncthreads();
      sum = shs[0];
      sum += shs[1]; sum += shs[2]; sum += shs[3];
      __syncthreads();
      const float inv = 1.0f / sum;
#pragma unroll
      for (int k = 0; k < PER; k++)
        if (col_of(k) < cols) yv[k] *= inv;
      if (y_out) {
        if (VEC) {
#pragma unroll
          for (int k4 = 0; k4 < PER / 4; k4++) {
            const int c = 4 * (tid + k4 * 256);
            if (c < cols) *reinterpret_cast<float4 *>(y_out + (long)r * ldyo + c) = make_float4(yv[4 * k4], yv[4 * k4 + 1], yv[4 * k4 + 2], yv[4 * k4 + 3]);
          }
        } else {
#pragma unroll
          for (int k = 0; k < PER; k++) {
            const int c = tid + k * 256;
            if (c < cols) y_out[(long)r * ldyo + c] = yv[k];
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < PER; k++) {
      const int c = col_of(k);
      if (c < cols) {
        if (!DENSE) tv[k] = (c == label ? 1.0f : 0.0f);
        tsum += tv[k];
        if (ybest < yv[k]) { ybest = yv[k]; yi = c; }
        if (tbest < tv[k]) { tbest = tv[k]; ti = c; }
      }
    }
    // diff (and the three sums' terms) from the posteriors in the registers.  wr = frame weight x sum(t): frames with sum(t) == 0 are switched
    // off (nnet-loss.cc:80-85).  With a label target sum(t) is 1 or 0 by the label alone -- known here, so the diff leaves BEFORE the block
    // reductions below (which then only feed the row's statistics) instead of behind them.
    double xe = 0.0, en = 0.0, lk = 0.0;
    auto emit = [&](const float wr) {
#pragma unroll
    for (int k = 0; k < PER; k++) {
      if (col_of(k) < cols) {
        const float yy = yv[k], tt = tv[k];
        yv[k] = (yy - tt) * wr;   // the diff, kept for the stores below
        if (tt != 0.0f) {  // t == 0 terms are exactly 0 (t*log(...) with finite log)
          xe += (double)(logf(yy + 1e-20f) * tt * wr);
          en += (double)(logf(tt + 1e-20f) * tt * wr);
          lk += (double)(yy * tt * wr);
        }
      }
    }
    if (VEC) {
#pragma unroll
      for (int k4 = 0; k4 < PER / 4; k4++) {
        const int c = 4 * (tid + k4 * 256);
        if (c < cols) {
          const float4 d4 = make_float4(yv[4 * k4], yv[4 * k4 + 1], yv[4 * k4 + 2], yv[4 * k4 + 3]);
          *reinterpret_cast<float4 *>(diff + (long)r * ldd + c) = d4;
          if (po.hi) {
            half4 hi, lo;
            s16_split4(d4, pscale, &hi, &lo);
            *reinterpret_cast<half4 *>(po.hi + (long)r * po.ld + c) = hi;
            *reinterpret_cast<half4 *>(po.lo + (long)r * po.ld + c) = lo;
          }
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < PER; k++) {
        const int c = tid + k * 256;
        if (c < cols) {
          diff[(long)r * ldd + c] = yv[k];
          if (po.hi) {
            h16 h, l;
            s16_split(yv[k], pscale, &h, &l);
            po.hi[(long)r * po.ld + c] = h;
            po.lo[(long)r * po.ld + c] = l;
          }
        }
      }
    }
    };
    const float tsum_by_label = (label >= 0 && label < cols) ? 1.0f : 0.0f;
    if (!DENSE) emit(fw_r * tsum_by_label);
    // block reductions: argmax(y); with dense targets also tsum and argmax(t) -- a label target's are known: sum 1 or 0, arg-max the label
    // (column 0 for a row of zeros: the lowest index among equals)
    if (DENSE) tsum = wave_sum(tsum);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      float ov = __shfl_xor(ybest, o, 64); int oi = __shfl_xor(yi, o, 64);
      if (ov > ybest || (ov == ybest && oi >= 0 && (yi < 0 || oi < yi))) { ybest = ov; yi = oi; }
      if (DENSE) {
        ov = __shfl_xor(tbest, o, 64); oi = __shfl_xor(ti, o, 64);
        if (ov > tbest || (ov == tbest && oi >= 0 && (ti < 0 || oi < ti))) { tbest = ov; ti = oi; }
      }
    }
    if (lane == 0) { shf[w][0] = tsum; shf[w][1] = ybest; shf[w][2] = tbest; shi[w][0] = yi; shi[w][1] = ti; }
    __syncthreads();
    if (SPARSE) {   // every thread has read its slots: the staging row back to zeros (the barriers below stand before the next row's entries)
      if (e_col >= 0 && e_col < cols) stage[e_col] = 0.0f;
      for (int i = e_next; i < e_end; i += 256) {
        const int c = labels[i];
        if (c >= 0 && c < cols) stage[c] = 0.0f;
      }
    }
    tsum = shf[0][0] + shf[1][0] + shf[2][0] + shf[3][0];
    ybest = shf[0][1]; yi = shi[0][0]; tbest = shf[0][2]; ti = shi[0][1];
#pragma unroll
    for (int j = 1; j < 4; j++) {
      if (shf[j][1] > ybest || (shf[j][1] == ybest && shi[j][0] >= 0 && (yi < 0 || shi[j][0] < yi))) { ybest = shf[j][1]; yi = shi[j][0]; }
      if (DENSE && (shf[j][2] > tbest || (shf[j][2] == tbest && shi[j][1] >= 0 && (ti < 0 || shi[j][1] < ti)))) { tbest = shf[j][2]; ti = shi[j][1]; }
    }
    if (!DENSE) { tsum = tsum_by_label; ti = (label >= 0 && label < cols) ? label : 0; }
    __syncthreads();
    const float wr = fw_r * tsum;
    if (DENSE) emit(wr);
    double *rs = rowstats + (long)r * 5;
    if (DENSE) {
      xe = wave_sum_d(xe); en = wave_sum_d(en); lk = wave_sum_d(lk);
      __shared__ double shd[4][3];
      if (lane == 0) { shd[w][0] = xe; shd[w][1] = en; shd[w][2] = lk; }
      __syncthreads();
      if (tid == 0) {
        rs[0] = (double)wr;
        rs[1] = (double)wr * (yi == ti ? 1.0 : 0.0);
        rs[2] = shd[0][0] + shd[1][0] + shd[2][0] + shd[3][0];
        rs[3] = shd[0][1] + shd[1][1] + shd[2][1] + shd[3][1];
        rs[4] = shd[0][2] + shd[1][2] + shd[2][2] + shd[3][2];
      }
    } else {
      // a label target has ONE non-zero term, in the thread that holds the label's column: that thread's three sums ARE the row's (every
      // other thread's are +0.0, and x + 0.0 = x), so they go out as they are -- no reduction over the workgroup
      const bool has_label = label >= 0 && label < cols;
      const bool mine = has_label && (VEC ? ((label >> 2) & 255) == tid : (label & 255) == tid);
      if (mine) { rs[2] = xe; rs[3] = en; rs[4] = lk; }
      if (tid == 0) {
        rs[0] = (double)wr;
        rs[1] = (double)wr * (yi == ti ? 1.0 : 0.0);
        if (!has_label) { rs[2] = 0.0; rs[3] = 0.0; rs[4] = 0.0; }
      }
    }
    __syncthreads();
  }
}

// The same for rows of any width (more than 256 * kXentPerThread classes): nothing is cached in registers, the row is streamed twice
// (targets: sum and both arg-maxes; then diff and the three sums).  Every thread visits the columns tid, tid + 256, ... in the same
// order and the reductions are those of the kernel above, so the result does not depend on which of the two kernels served a row.
template <bool DENSE>
__global__ void __launch_bounds__(256) xent_rows_wide_kernel(const float *y, int ldy, const float *t, int ldt, const int32_t *labels, const float *fw,
                                                             float *diff, int ldd, int rows, int cols, double *rowstats) {
  __shared__ float shf[4][4];
  __shared__ int shi[4][2];
  __shared__ double shd[4][3];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int r = blockIdx.x; r < rows; r += gridDim.x) {
    const float *yr = y + (long)r * ldy;
    const float *tr = DENSE ? t + (long)r * ldt : nullptr;
    const int label = DENSE ? -1 : labels[r];
    float tsum = 0.0f, ybest = -1e21f, tbest = -1e21f;
    int yi = -1, ti = -1;
    for (int c = tid; c < cols; c += 256) {
      const float yy = yr[c], tt = DENSE ? tr[c] : (c == label ? 1.0f : 0.0f);
      tsum += tt;
      if (ybest < yy) { ybest = yy; yi = c; }
      if (tbest < tt) { tbest = tt; ti = c; }
    }
    tsum = wave_sum(tsum);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      float ov = __shfl_xor(ybest, o, 64); int oi = __shfl_xor(yi, o, 64);
      if (ov > ybest || (ov == ybest && oi >= 0 && (yi < 0 || oi < yi))) { ybest = ov; yi = oi; }
      ov = __shfl_xor(tbest, o, 64); oi = __shfl_xor(ti, o, 64);
      if (ov > tbest || (ov == tbest && oi >= 0 && (ti < 0 || oi < ti))) { tbest = ov; ti = oi; }
    }
    if (lane == 0) { shf[w][0] = tsum; shf[w][1] = ybest; shf[w][2] = tbest; shi[w][0] = yi; shi[w][1] = ti; }
    __syncthreads();
    tsum = shf[0][0] + shf[1][0] + shf[2][0] + shf[3][0];
    ybest = shf[0][1]; yi = shi[0][0]; tbest = shf[0][2]; ti = shi[0][1];
#pragma unroll
    for (int j = 1; j < 4; j++) {
      if (shf[j][1] > ybest || (shf[j][1] == ybest && shi[j][0] >= 0 && (yi < 0 || shi[j][0] < yi))) { ybest = shf[j][1]; yi = shi[j][0]; }
      if (shf[j][2] > tbest || (shf[j][2] == tbest && shi[j][1] >= 0 && (ti < 0 || shi[j][1] < ti))) { tbest = shf[j][2]; ti = shi[j][1]; }
    }
    __syncthreads();
    const float wr = fw[r] * tsum;
    double xe = 0.0, en = 0.0, lk = 0.0;
    for (int c = tid; c < cols; c += 256) {
      const float yy = yr[c], tt = DENSE ? tr[c] : (c == label ? 1.0f : 0.0f);
      diff[(long)r * ldd + c] = (yy - tt) * wr;
      if (tt != 0.0f) {
        xe += (double)(logf(yy + 1e-20f) * tt * wr);
        en += (double)(logf(tt + 1e-20f) * tt * wr);
        lk += (double)(yy * tt * wr);
      }
    }
    xe = wave_sum_d(xe); en = wave_sum_d(en); lk = wave_sum_d(lk);
    if (lane == 0) { shd[w][0] = xe; shd[w][1] = en; shd[w][2] = lk; }
    __syncthreads();
    if (tid == 0) {
      double *rs = rowstats + (long)r * 5;
      rs[0] = (double)wr;
      rs[1] = (double)wr * (yi == ti ? 1.0 : 0.0);
      rs[2] = shd[0][0] + shd[1][0] + shd[2][0] + shd[3][0];
      rs[3] = shd[0][1] + shd[1][1] + shd[2][1] + shd[3][1];
      rs[4] = shd[0][2] + shd[1][2] + shd[2][2] + shd[3][2];
    }
    __syncthreads();
  }
}

// stats[0..4] += {frames, correct, xent, entropy, likelihood}; fixed-order sum over rows
__global__ void __launch_bounds__(256) xent_finalize_kernel(const double *rowstats, int rows, double *stats) { xent_sum_rows(rowstats, rows, stats, false); }
// The same for the per-row statistics of several batches at once (aslp_xent_sum_rowstats): workgroup b sums batch b exactly as above, then
// one thread adds the batches' sums to the accumulators in batch order -- the bits of one xent_finalize_kernel launch per batch.
__global__ void __launch_bounds__(256) xent_batch_sums_kernel(const double *rowstats, int rows, double *sums) {
  xent_sum_rows<true>(rowstats + (size_t)blockIdx.x * rows * 5, rows, sums + (size_t)blockIdx.x * 5, false);
}
__global__ void xent_apply_kernel(const double *sums, int batches, double *stats) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double a[5] = {stats[0], stats[1], stats[2], stats[3], stats[4]};
  for (int b = 0; b < batches; b++) {
    const double *s = sums + (size_t)b * 5;
    a[0] += s[0]; a[1] += s[1]; a[2] += -s[2]; a[3] += -s[3]; a[4] += s[4];
  }
  for (int k = 0; k < 5; k++) stats[k] = a[k];
}

// ---- Mse ------------------------------------------------------------------------------
// Mse::Eval in one pass over net_out and the targets (aslp_mse_eval).  One wave per row, four rows per workgroup at a time, at most 256
// workgroups (the maxima array of aslp_planes_out holds that many); a lane takes the row's columns (VEC: its groups of four columns) lane,
// lane + 64, ...  Per element, every operation rounded on its own: e = (y - t) w, diff = e (or e * scale), q = (e e) w -- the bits of
// AddMat(-1), MulRowsVec, [Scale], MulElements, MulRowsVec.  row_loss[r] = sum of the row's q in double: a lane's columns in rising
// order, then the wave's butterfly -- the same order in every call, no atomics.  parts (nullable): the workgroup's largest finite |diff|.
// VEC: 16-byte accesses; the group that holds a row's last column is read and written column by column (s16_load4_ragged), so neither
// form touches a float at a column >= cols (row padding, or the neighbouring task's columns of a MultiTask window).
// frames_out (nullable): one more workgroup, the launch's last, leaves trunc(sum of the weights, in index order, in double) there.
template <bool VEC>
__global__ void __launch_bounds__(kPanelThreads) mse_rows_kernel(const float *y, int ldy, const float *t, int ldt, const float *__restrict__ fw,
                                                                 float scale, float *diff, int ldd, int rows, int cols,
                                                                 double *__restrict__ row_loss, float *__restrict__ parts,
                                                                 double *__restrict__ frames_out) {
#pragma clang fp contract(off)
  __shared__ float red[kPanelWaves];
  const int nwg = frames_out != nullptr ? (int)gridDim.x - 1 : (int)gridDim.x;
  if ((int)blockIdx.x == nwg) {   // (uniform: the whole workgroup)
    if (threadIdx.x == 0) {
      double s = 0.0;
      for (int r = 0; r < rows; r++) s += (double)fw[r];
      frames_out[0] = trunc(s);
    }
    return;
  }
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const bool scaled = scale != 1.0f;
  float m = 0.f;
  for (int r = (int)blockIdx.x * kPanelWaves + wave; r < rows; r += nwg * kPanelWaves) {
    const float w = fw[r];
    const float *yr = y + (long)r * ldy, *tr = t + (long)r * ldt;
    float *dr = diff + (long)r * ldd;
    double acc = 0.0;
    if constexpr (VEC) {
      const int c4 = (cols + 3) >> 2;
      for (int g = lane; g < c4; g += kWave) {
        const int c = 4 * g;
        const float4 yv = s16_load4_ragged(yr, c, cols), tv = s16_load4_ragged(tr, c, cols);
        const float ya[4] = {yv.x, yv.y, yv.z, yv.w}, ta[4] = {tv.x, tv.y, tv.z, tv.w};
        float d[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const float e = (ya[i] - ta[i]) * w;
          d[i] = scaled ? e * scale : e;
          const float q = (e * e) * w;
          if (c + i < cols) acc += (double)q;
        }
        if (c + 4 <= cols) {
          const float4 dv = make_float4(d[0], d[1], d[2], d[3]);
          m = s16_absmax4(m, dv);
          *reinterpret_cast<float4 *>(dr + c) = dv;
        } else {   // (the row ends inside this group: nothing is written behind its last column, nothing behind it counts)
          for (int i = 0; i < 4 && c + i < cols; i++) {
            const float a = fabsf(d[i]);
            m = fmaxf(m, a < 3.0e38f ? a : 0.f);
            dr[c + i] = d[i];
          }
        }
      }
    } else {
      for (int c = lane; c < cols; c += kWave) {
        const float e = (yr[c] - tr[c]) * w;
        const float dv = scaled ? e * scale : e;
        const float q = (e * e) * w;
        acc += (double)q;
        const float a = fabsf(dv);
        m = fmaxf(m, a < 3.0e38f ? a : 0.f);
        dr[c] = dv;
      }
    }
    acc = wave_sum_d(acc);
    if (lane == 0) row_loss[r] = acc;
  }
  if (parts != nullptr) {   // (uniform)
    m = wg_max(m, red);
    if (threadIdx.x == 0) parts[blockIdx.x] = m;
  }
}
// What Mse parks batch after batch (aslp_mse_eval's row_loss, `rows` doubles, and one double behind them: the batch's frame count where the
// device formed it) summed per batch: sums[2 b] = the batch's loss sum (thread t: rows t, t + 256, ... in rising order; the wave's
// butterfly; the four waves in order), sums[2 b + 1] = the double behind its rows.  One workgroup per batch.
__global__ void __launch_bounds__(256) mse_batch_sums_kernel(const double *pending, int rows, double *sums) {
  __shared__ double sh[4];
  const double *p = pending + (size_t)blockIdx.x * ((size_t)rows + 1);
  double a = 0.0;
  for (int r = threadIdx.x; r < rows; r += 256) a += p[r];
  a = wave_sum_d(a);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    sums[2 * (size_t)blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    sums[2 * (size_t)blockIdx.x + 1] = p[rows];
  }
}

// ---- Xent over column blocks (MultiTaskLoss over BlockSoftmax) ---------------------------------------------------------------
// aslp_xent_blocks_eval: per (row, block) the block's softmax, the labelled Xent diff and row statistics, the task weight and
// BlockSoftmax' backward mask, in one launch.  The block table travels by value.
constexpr int kXbMaxBlocks = 16;
constexpr int kXbWaveCols = 512;   // up to here one wave holds a block's row (launch_softmax' first rung)
struct XbArgs {
  int n;
  int off[kXbMaxBlocks], cols[kXbMaxBlocks];
  float weight[kXbMaxBlocks];
  double *rs[kXbMaxBlocks];
  unsigned vec;    // bit b: block b's activations (and posteriors out) take the 16-byte map
  unsigned dvec;   // bit b: ... and its diff rows allow 16-byte stores
};
struct XbShared {
  float f[4];
  float best[4];
  int idx[4];
};

// One block of one row, held in the registers of NT threads from load to store: NT = 64, a wave (column lane + 64 k, the map of
// softmax_rows_kernel<64>), or NT = 256, the workgroup (xent_rows_kernel's two maps).  The softmax is softmax_rows_kernel's arithmetic in
// its order; diff, statistics and arg-max are those of xent_rows_kernel's label form.  The mask's row sum: a thread's slots in slot
// order, the wave's butterfly, then (NT = 256) the four waves in order.  Returns the thread's largest finite |diff|.
template <int NT, int PER, bool VEC>
__device__ __forceinline__ float xb_block(const float *yr, const int cols, const int label, const float fw_r, const float weight, float *dr,
                                          const bool dvec, float *pr, const bool softmax, const bool mask, double *rs, XbShared *sh) {
#pragma clang fp contract(off)
  static_assert(!VEC || (NT == 256 && PER % 4 == 0), "the 16-byte map is for whole-workgroup rows");
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int t = NT == 64 ? lane : (int)threadIdx.x;
  auto col_of = [t](int k) { return VEC ? 4 * (t + (k >> 2) * NT) + (k & 3) : t + k * NT; };
  float yv[PER];
  if (VEC) {
#pragma unroll
    for (int k4 = 0; k4 < PER / 4; k4++) {
      const int c = 4 * (t + k4 * NT);
      if (c < cols) {
        const float4 v4 = *reinterpret_cast<const float4 *>(yr + c);
        yv[4 * k4] = v4.x; yv[4 * k4 + 1] = v4.y; yv[4 * k4 + 2] = v4.z; yv[4 * k4 + 3] = v4.w;
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < PER; k++) {
      const int c = t + k * NT;
      if (c < cols) yv[k] = yr[c];
    }
  }
  if (softmax) {
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < PER; k++)
      if (col_of(k) < cols) m = fmaxf(m, yv[k]);
    m = wave_max(m);
    if (NT == 256) {
      if (lane == 0) sh->f[w] = m;
      __syncthreads();
      m = fmaxf(fmaxf(fmaxf(sh->f[0], sh->f[1]), sh->f[2]), sh->f[3]);
      __syncthreads();
    }
    float sum = 0.0f;
#pragma unroll
    for (int k = 0; k < PER; k++) {
      if (col_of(k) < cols) {
        yv[k] = expf(yv[k] - m);
        sum += yv[k];
      }
    }
    sum = wave_sum(sum);
    if (NT == 256) {
      if (lane == 0) sh->f[w] = sum;
      __syncthreads();
      sum = sh->f[0];
      sum += sh->f[1]; sum += sh->f[2]; sum += sh->f[3];
      __syncthreads();
    }
    const float inv = 1.0f / sum;
#pragma unroll
    for (int k = 0; k < PER; k++)
      if (col_of(k) < cols) yv[k] *= inv;
  }
  if (pr) {
    if (VEC) {
#pragma unroll
      for (int k4 = 0; k4 < PER / 4; k4++) {
        const int c = 4 * (t + k4 * NT);
        if (c < cols) *reinterpret_cast<float4 *>(pr + c) = make_float4(yv[4 * k4], yv[4 * k4 + 1], yv[4 * k4 + 2], yv[4 * k4 + 3]);
      }
    } else {
#pragma unroll
      for (int k = 0; k < PER; k++) {
        const int c = t + k * NT;
        if (c < cols) pr[c] = yv[k];
      }
    }
  }
  // the label is compared with column numbers only, never added to a pointer
  const bool has_label = label >= 0 && label < cols;
  const float wr = fw_r * (has_label ? 1.0f : 0.0f);
  float ybest = -1e21f;
  int yi = -1;
  double xe = 0.0, en = 0.0, lk = 0.0;
  float s = 0.0f;
#pragma unroll
  for (int k = 0; k < PER; k++) {
    const int c = col_of(k);
    if (c < cols) {
      const float yy = yv[k], tt = (c == label ? 1.0f : 0.0f);
      if (ybest < yy) { ybest = yy; yi = c; }
      const float e = (yy - tt) * wr;
      if (tt != 0.0f) {
        xe += (double)(logf(yy + 1e-20f) * tt * wr);
        en += (double)(logf(tt + 1e-20f) * tt * wr);
        lk += (double)(yy * tt * wr);
      }
      yv[k] = weight != 1.0f ? e * weight : e;
      s += yv[k];
    }
  }
  if (mask) {
    s = wave_sum(s);
    if (NT == 256) {
      if (lane == 0) sh->f[w] = s;
      __syncthreads();
      s = sh->f[0];
      s += sh->f[1]; s += sh->f[2]; s += sh->f[3];
      __syncthreads();
    }
    const float f = 1.0f - s;
#pragma unroll
    for (int k = 0; k < PER; k++)
      if (col_of(k) < cols) yv[k] *= f;
  }
  float amax = 0.f;
#pragma unroll
  for (int k = 0; k < PER; k++)
    if (col_of(k) < cols) {
      const float a = fabsf(yv[k]);
      amax = fmaxf(amax, a < 3.0e38f ? a : 0.f);
    }
  if (VEC && dvec) {
#pragma unroll
    for (int k4 = 0; k4 < PER / 4; k4++) {
      const int c = 4 * (t + k4 * NT);
      if (c < cols) *reinterpret_cast<float4 *>(dr + c) = make_float4(yv[4 * k4], yv[4 * k4 + 1], yv[4 * k4 + 2], yv[4 * k4 + 3]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < PER; k++) {
      const int c = col_of(k);
      if (c < cols) dr[c] = yv[k];
    }
  }
  // arg-max of the posteriors: the lowest index among equals, as xent_rows_kernel finds it
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(ybest, o, 64);
    const int oi = __shfl_xor(yi, o, 64);
    if (ov > ybest || (ov == ybest && oi >= 0 && (yi < 0 || oi < yi))) { ybest = ov; yi = oi; }
  }
  if (NT == 256) {
    if (lane == 0) { sh->best[w] = ybest; sh->idx[w] = yi; }
    __syncthreads();
    ybest = sh->best[0]; yi = sh->idx[0];
#pragma unroll
    for (int j = 1; j < 4; j++)
      if (sh->best[j] > ybest || (sh->best[j] == ybest && sh->idx[j] >= 0 && (yi < 0 || sh->idx[j] < yi))) { ybest = sh->best[j]; yi = sh->idx[j]; }
    __syncthreads();
  }
  const int ti = has_label ? label : 0;
  // a label target has one non-zero term, in the thread that holds the label's column: its three sums are the row's
  const bool mine = has_label && (VEC ? ((label >> 2) & (NT - 1)) == t : (label & (NT - 1)) == t);
  if (mine) { rs[2] = xe; rs[3] = en; rs[4] = lk; }
  if (t == 0) {
    rs[0] = (double)wr;
    rs[1] = (double)wr * (yi == ti ? 1.0 : 0.0);
    if (!has_label) { rs[2] = 0.0; rs[3] = 0.0; rs[4] = 0.0; }
  }
  return amax;
}

// One workgroup per row, workgroup b of the g <= 256 takes rows b, b + g, ...  Blocks wider than 512 columns take the whole workgroup,
// one after the other (PER: the slots of the widest); then wave w serves the narrower blocks w, w + 4, ... of those, no barrier between
// them.  parts[b] (nullable): the largest finite |diff| of the workgroup's rows.
template <int PER>
__global__ void __launch_bounds__(256) xent_blocks_kernel(const float *in, int ldi, XbArgs a, const int32_t *labels, const float *fw, float *diff, int ldd,
                                                          int rows, int softmax, int mask, float *post, int ldp, float *parts) {
  __shared__ XbShared sh;
  __shared__ float red[kPanelWaves];
  const int wave = threadIdx.x >> 6;
  float amax = 0.f;
  for (int r = blockIdx.x; r < rows; r += gridDim.x) {
    const float fw_r = fw[r];
    const float *ir = in + (long)r * ldi;
    float *dr = diff + (long)r * ldd;
    float *pr = post != nullptr ? post + (long)r * ldp : nullptr;
    const int32_t *lr = labels + (long)r * a.n;
    for (int b = 0; b < a.n; b++) {   // (uniform: the table is the launch's)
      if (a.cols[b] <= kXbWaveCols) continue;
      double *rs = a.rs[b] + (long)r * 5;
      float *pb = pr != nullptr ? pr + a.off[b] : nullptr;
      float m;
      if ((a.vec >> b) & 1u)
        m = xb_block<256, PER, true>(ir + a.off[b], a.cols[b], lr[b], fw_r, a.weight[b], dr + a.off[b], ((a.dvec >> b) & 1u) != 0, pb, softmax != 0, mask != 0, rs, &sh);
      else
        m = xb_block<256, PER, false>(ir + a.off[b], a.cols[b], lr[b], fw_r, a.weight[b], dr + a.off[b], false, pb, softmax != 0, mask != 0, rs, &sh);
      amax = fmaxf(amax, m);
    }
    int narrow = 0;
    for (int b = 0; b < a.n; b++) {
      if (a.cols[b] > kXbWaveCols) continue;
      if ((narrow++ & 3) != wave) continue;
      const float m = xb_block<64, kXbWaveCols / 64, false>(ir + a.off[b], a.cols[b], lr[b], fw_r, a.weight[b], dr + a.off[b], false,
                                                             pr != nullptr ? pr + a.off[b] : nullptr, softmax != 0, mask != 0, a.rs[b] + (long)r * 5, nullptr);
      amax = fmaxf(amax, m);
    }
  }
  if (parts != nullptr) {   // (uniform)
    amax = wg_max(amax, red);
    if (threadIdx.x == 0) parts[blockIdx.x] = amax;
  }
}

}  // namespace

static bool g_coop_convert_on = true;   // aslp_coop_convert (tests: the two-launch conversion as the reference)
// split16.h: (optional copy and) planes of n matrices in one launch; false = not served, nothing was launched
bool coop_convert_launch(const CoopConvJob *jobs, int n, const SeqFillJob *fill) {
  static const bool off = [] { const char *e = getenv("ASLP_COPY_PLANES"); return e != nullptr && e[0] == '0'; }();   // A/B switch
  // Not beside the main stream: a launch there may share the chip with a persistent recurrence whose workgroups need every CU (each
  // would wait for workgroups the other keeps from being placed), and two launches of this thread would meet in one exchange area.
  if (off || !g_coop_convert_on || n <= 0 || n > kS16MaxJobs) return false;
  long max_units = 0;
  bool ragged = false;   // a width that is no multiple of 4: only under gemm_split16_ragged(), on the kernel's ragged form
  CoopConvJobs js;
  for (int i = 0; i < n; i++) {
    const CoopConvJob &c = jobs[i];
    if (!c.src || !c.pl.hi || !c.pl.lo || !c.pl.slot || c.pl.rows <= 0 || c.pl.cols <= 0 || ((c.pl.cols & 3) && !gemm_split16_ragged()) || (c.ld_src & 3) ||
        !aligned16(c.src) || (c.dst && ((c.ld_dst & 3) || !aligned16(c.dst))) || c.pl.ld < c.pl.cols || (c.pl.ld & 3) || (c.parts && c.nparts <= 0))
      return false;
    ragged = ragged || (c.pl.cols & 3);
    max_units = std::max(max_units, (long)c.pl.rows * ((c.pl.cols + 3) >> 2));
    js.j[i] = c;
  }
  CoopState &st = coop_state();
  if (!st.gmax || !coop_grid_wide_ok()) return false;
  // every workgroup of the launch resident at once (those of a matrix wait for each other): at most two per CU (four fit by registers and
  // wave slots; beside a layer product's workgroup, one -- the second then waits for that workgroup to end, which it does)
  const int cus = std::min(2 * coop_cu_count(), kCoopGmaxWords);
  int U = 0, gx = 0;
  for (int u : {4, 8, 16}) {
    const long g = (max_units + (long)u * kPanelThreads - 1) / ((long)u * kPanelThreads);
    if (U == 0 && g * n <= cus) { U = u; gx = (int)g; }
  }
  if (U == 0) return false;
  if (++st.token == 0) st.token = 1;
  SeqFillJob fj = {nullptr, nullptr, 0, 0, 0, 0, 0, nullptr, 0, 0};
  if (fill) fj = *fill;
#define ASLP_COPY_PLANES_R(UU, RG) hipLaunchKernelGGL((copy_planes_coop<UU, RG>), dim3(gx, n), dim3(kPanelThreads), 0, cur_stream(), js, st.gmax, st.token, st.err, fj)
#define ASLP_COPY_PLANES(UU) do { if (ragged) ASLP_COPY_PLANES_R(UU, true); else ASLP_COPY_PLANES_R(UU, false); } while (0)
  if (U == 4) ASLP_COPY_PLANES(4); else if (U == 8) ASLP_COPY_PLANES(8); else ASLP_COPY_PLANES(16);
#undef ASLP_COPY_PLANES_R
#undef ASLP_COPY_PLANES
  check_launch("coop_convert");
  return true;
}
}  // namespace aslp

using namespace aslp;

extern "C" {

void aslp_bn_forward_act(const float *in, MatrixDim d, float *out, int out_stride, float *xhat, int xhat_stride, const float *scale,
                         const float *shift, float *mean, float *inv_std, double *acc_means, double *acc_vars, float var_floor, float *act_out,
                         int act_stride) {
  if (d.rows <= 0 || d.cols <= 0) return;
  if (!out && !act_out) { set_error("aslp_bn_forward: no output"); return; }
  const float invB = 1.0f / (float)d.rows;
  const bool in_vec = vec_ok(in, d.stride);
  const bool vec = d.cols % 4 == 0 && in_vec && (!out || vec_ok(out, out_stride)) && (!xhat || vec_ok(xhat, xhat_stride)) &&
                   (!act_out || vec_ok(act_out, act_stride)) && vec_ok(mean) && vec_ok(inv_std) && vec_ok(scale) && vec_ok(shift);
  const BnPath bp = bn_path_for(d.rows, d.cols, vec);
  const dim3 block(kPanelThreads);
  if (bp.path == 2) {
    CoopState &st = coop_state();
    const dim3 grid((d.cols / kCoopCols) * bp.q);
    with_slots(bp.slots, [&](auto S) {
      hipLaunchKernelGGL((bn_forward_coop<decltype(S)::value>), grid, block, 0, cur_stream(), in, d.stride, out, out_stride, xhat, xhat_stride, scale, shift,
                         mean, inv_std, acc_means, acc_vars, invB, var_floor, d.rows, act_out, act_stride, bp.q, st.inbox, st.err);
    });
    check_launch("bn_forward_coop");
    return;
  }
  if (bp.path == 1) {
    const dim3 grid(d.cols / (4 * kPanelCG));
    with_slots(bp.slots, [&](auto S) {
      hipLaunchKernelGGL((bn_forward_panel<kPanelCG, decltype(S)::value>), grid, block, 0, cur_stream(), in, d.stride, out, out_stride, xhat, xhat_stride,
                         scale, shift, mean, inv_std, acc_means, acc_vars, invB, var_floor, d.rows, act_out, act_stride);
    });
    check_launch("bn_forward_panel");
    return;
  }
  colreduce<3, double>("bn_forward.stats", d.rows, d.cols, BnSum1F{in, d.stride}, BnSum1G{invB, var_floor, d.rows, mean, inv_std, acc_means, acc_vars},
                       in_vec);
  long n = (long)d.rows * (vec ? d.cols / 4 : d.cols);
  if (vec) hipLaunchKernelGGL((bn_normalize_kernel<true>), dim3(grid_for(n)), dim3(kBlock), 0, cur_stream(), in, d.stride, out, out_stride, xhat, xhat_stride, mean, inv_std, scale, shift, d.rows, d.cols, act_out, act_stride);
  else hipLaunchKernelGGL((bn_normalize_kernel<false>), dim3(grid_for(n)), dim3(kBlock), 0, cur_stream(), in, d.stride, out, out_stride, xhat, xhat_stride, mean, inv_std, scale, shift, d.rows, d.cols, act_out, act_stride);
  check_launch("bn_forward");
}
int aslp_bn_forward_stats(const float *in, MatrixDim d, float *out, int out_stride, const float *scale, const float *shift, float *mean,
                          float *inv_std, double *acc_means, double *acc_vars, float var_floor, float *act_out, int act_stride,
                          const double *colstats, int groups, int stats_ld) {
  return aslp_bn_forward_stats_p(in, d, out, out_stride, scale, shift, mean, inv_std, acc_means, acc_vars, var_floor, act_out, act_stride, colstats,
                                 groups, stats_ld, nullptr);
}
int aslp_bn_forward_stats_p(const float *in, MatrixDim d, float *out, int out_stride, const float *scale, const float *shift, float *mean,
                            float *inv_std, double *acc_means, double *acc_vars, float var_floor, float *act_out, int act_stride,
                            const double *colstats, int groups, int stats_ld, const aslp_planes_out *act_planes) {
  if (d.rows <= 0 || d.cols <= 0 || !colstats) return 0;
  if (!out && !act_out) { set_error("aslp_bn_forward_stats: no output"); return 0; }
  if (groups != (d.rows + 31) / 32 || stats_ld < d.cols) { set_error("aslp_bn_forward_stats: statistics layout does not match the matrix"); return 0; }
  static const bool off = [] { const char *e = getenv("ASLP_BN_FROM_STATS"); return e && e[0] == '0'; }();   // A/B switch
  const bool vec = d.cols % 4 == 0 && vec_ok(in, d.stride) && (!out || vec_ok(out, out_stride)) && (!act_out || vec_ok(act_out, act_stride)) && vec_ok(mean) &&
                   vec_ok(inv_std) && vec_ok(scale) && vec_ok(shift);
  // the shapes the backward pass serves without a stored normalised copy (it recomputes xhat from `in` and the batch mean)
  if (off || !vec || d.cols % kCoopCols != 0 || !bn_panel_shape(d.rows, d.cols)) return 0;
  const int P = d.cols / kCoopCols;
  int Q = 1;
  while (Q < 8 && P * Q * 2 <= 1024 && (d.rows + 2 * Q - 1) / (2 * Q) >= 64) Q *= 2;   // ~4 workgroups per CU at most, >= 64 rows each
  while ((d.rows + Q - 1) / Q > kStatSlots * kCoopLanes) Q *= 2;                       // at most kStatSlots rows per thread
  S16Out po = {nullptr, nullptr, 0, nullptr, nullptr};
  if (act_planes && act_planes->hi && act_out && act_planes->slot && act_planes->ld >= d.cols)
    po = S16Out{static_cast<h16 *>(act_planes->hi), static_cast<h16 *>(act_planes->lo), act_planes->ld, act_planes->slot, nullptr};
  hipLaunchKernelGGL(bn_forward_stats_kernel, dim3(P * Q), dim3(kPanelThreads), 0, cur_stream(), in, d.stride, out, out_stride, scale, shift, mean,
                     inv_std, acc_means, acc_vars, 1.0f / (float)d.rows, var_floor, d.rows, act_out, act_stride, Q, colstats, groups, stats_ld, po);
  check_launch("bn_forward_stats");
  return 1;
}

void aslp_bn_forward(const float *in, MatrixDim d, float *out, int out_stride, float *xhat, int xhat_stride, const float *scale,
                     const float *shift, float *mean, float *inv_std, double *acc_means, double *acc_vars, float var_floor) {
  aslp_bn_forward_act(in, d, out, out_stride, xhat, xhat_stride, scale, shift, mean, inv_std, acc_means, acc_vars, var_floor, nullptr, 0);
}

void aslp_bn_apply(const float *in, MatrixDim d, float *out, int out_stride, const float *mean, const float *inv_std, const float *scale, const float *shift) {
  if (d.rows <= 0 || d.cols <= 0) return;
  long n = (long)d.rows * d.cols;
  hipLaunchKernelGGL((bn_normalize_kernel<false>), dim3(grid_for(n)), dim3(kBlock), 0, cur_stream(), in, d.stride, out, out_stride, (float *)nullptr, 0, mean, inv_std, scale, shift, d.rows, d.cols, (float *)nullptr, 0);
  check_launch("bn_apply");
}

// A batch of one row has no gradient through the normalisation: x - mean is zero and in_diff = D inv_std - inv_std D, which the reference
// forms from one rounded product and so gets exactly 0.  The write passes add D inv_std to a separately rounded -inv_std scale S1 / rows
// and leave one ulp of those terms (inv_std = 1 / sqrt(floor) = 3162: 5e-4) where the result is zero.
static void bn_in_diff_one_row(MatrixDim d, float *in_diff) {
  if (d.rows == 1 && in_diff) ASLP_CHECK_HIP(hipMemsetAsync(in_diff, 0, sizeof(float) * (size_t)d.cols, cur_stream()));
}
static void bn_backward_impl(MatrixDim d, const float *out_diff, int od_stride, float *xhat, int xhat_stride, float *scale, float *shift,
                             const float *inv_std, float *dscale, float *dshift, float momentum, float *in_diff, int id_stride,
                             const float *act_y, int act_stride, bool step, float learn_rate, const float *in, const float *mean,
                             aslp_planes_out *diff_out = nullptr) {
  if (diff_out) { diff_out->nparts = 0; diff_out->planes_written = 0; }
  if (d.rows <= 0 || d.cols <= 0) return;
  const bool y_ok = !act_y || vec_ok(act_y, act_stride);
  const bool recompute = xhat == nullptr;
  if (recompute && (!in || !mean)) { set_error("aslp_bn_backward: without a normalised copy (xhat == NULL) the layer input and the batch mean are needed"); return; }
  const bool panel_ok = vec_ok(out_diff, od_stride) && (!in_diff || vec_ok(in_diff, id_stride)) && vec_ok(inv_std) && y_ok &&
                        (recompute ? (vec_ok(in, d.stride) && vec_ok(mean)) : vec_ok(xhat, xhat_stride));
  const BnPath bp = bn_path_for(d.rows, d.cols, panel_ok);
  if (!bp.path && recompute) { set_error("aslp_bn_backward: xhat == NULL is only served by the single-launch panel path (check aslp_bn_panel_supported)"); return; }
  const dim3 block(kPanelThreads);
  // the instantiation for (slots, act_y != NULL, recompute): f(SLOTS, HAS_Y, RECOMPUTE) as integral constants
  auto with_instantiation = [&](auto &&f) {
    with_slots(bp.slots, [&](auto S) { with_flag(act_y != nullptr, [&](auto Y) { with_flag(recompute, [&](auto R) { f(S, Y, R); }); }); });
  };
  if (bp.path == 2) {
    CoopState &st = coop_state();
    const dim3 grid((d.cols / kCoopCols) * bp.q);
    // in_diff's planes from this launch when all its workgroups are resident at once (they wait for each other's maxima: one per CU is
    // what the shape was chosen for), else the maxima for the conversion pass
    S16Out po = {nullptr, nullptr, 0, nullptr, nullptr};
    unsigned token = 0;
    static const bool planes_off = [] { const char *e = getenv("ASLP_BN_DIFF_PLANES"); return e != nullptr && e[0] == '0'; }();   // A/B switch
    if (diff_out && diff_out->hi && diff_out->lo && diff_out->slot && in_diff && st.gmax && !planes_off && coop_grid_wide_ok() && (int)grid.x <= kCoopGmaxWords &&
        (int)grid.x <= coop_cu_count() && diff_out->ld >= d.cols && diff_out->ld % 4 == 0) {
      po = S16Out{static_cast<h16 *>(diff_out->hi), static_cast<h16 *>(diff_out->lo), diff_out->ld, diff_out->slot, nullptr};
      if (++st.token == 0) st.token = 1;
      token = st.token;
      diff_out->planes_written = 1;
    }
    float *max_parts = (!po.hi && diff_out && diff_out->parts && in_diff && (int)grid.x <= kS16MaxParts) ? diff_out->parts : nullptr;
    if (max_parts) diff_out->nparts = (int)grid.x;
    with_instantiation([&](auto S, auto Y, auto R) {
      hipLaunchKernelGGL((bn_backward_coop<decltype(S)::value, decltype(Y)::value, decltype(R)::value>), grid, block, 0, cur_stream(), out_diff, od_stride, xhat,
                         xhat_stride, scale, shift, inv_std, dscale, dshift, momentum, -learn_rate, step, in_diff, id_stride, d.rows, act_y, act_stride, in,
                         d.stride, mean, bp.q, st.inbox, st.err, max_parts, po, st.gmax, token);
    });
    check_launch("bn_backward_coop");
    return;
  }
  if (bp.path == 1) {
    const dim3 grid(d.cols / (4 * kPanelCG));
    with_instantiation([&](auto S, auto Y, auto R) {
      hipLaunchKernelGGL((bn_backward_panel<kPanelCG, decltype(S)::value, decltype(Y)::value, decltype(R)::value>), grid, block, 0, cur_stream(), out_diff,
                         od_stride, xhat, xhat_stride, scale, shift, inv_std, dscale, dshift, momentum, -learn_rate, step, in_diff, id_stride, d.rows, act_y,
                         act_stride, in, d.stride, mean);
    });
    check_launch("bn_backward_panel");
    bn_in_diff_one_row(d, in_diff);
    return;
  }
  float *s12 = static_cast<float *>(scratch(kScratchReduce2, sizeof(float) * 3 * (size_t)d.cols));
  if (!s12) return;
  float *scale_used = s12 + 2 * (size_t)d.cols;
  const bool stats_vec = vec_ok(out_diff, od_stride) && vec_ok(xhat, xhat_stride) && y_ok;
  colreduce<2, float>("bn_backward.stats", d.rows, d.cols, BnBwdF{out_diff, od_stride, xhat, xhat_stride, act_y, act_stride},
                      BnBwdG{momentum, dscale, dshift, s12, s12 + d.cols, scale, shift, scale_used, -learn_rate, step}, stats_vec);
  if (!in_diff) return;
  long n = (long)d.rows * d.cols;
  const bool vec = d.cols % 4 == 0 && stats_vec && vec_ok(in_diff, id_stride) && vec_ok(inv_std) && vec_ok(s12);
  if (vec) hipLaunchKernelGGL((bn_backward_kernel<true>), dim3(grid_for(n / 4)), dim3(kBlock), 0, cur_stream(), out_diff, od_stride, xhat, xhat_stride, scale_used, inv_std, s12, s12 + d.cols, in_diff, id_stride, d.rows, d.cols, act_y, act_stride);
  else hipLaunchKernelGGL((bn_backward_kernel<false>), dim3(grid_for(n)), dim3(kBlock), 0, cur_stream(), out_diff, od_stride, xhat, xhat_stride, scale_used, inv_std, s12, s12 + d.cols, in_diff, id_stride, d.rows, d.cols, act_y, act_stride);
  check_launch("bn_backward");
  bn_in_diff_one_row(d, in_diff);
}
void aslp_bn_backward_act(const float *in, MatrixDim d, const float *out_diff, int od_stride, float *xhat, int xhat_stride, const float *scale,
                          const float *mean, const float *inv_std, float *dscale, float *dshift, float momentum, float *in_diff, int id_stride,
                          const float *act_y, int act_stride) {
  // with xhat: (x - mean) is recovered as xhat / inv_std; without (panel path only): x_hat is formed again from `in` and `mean`
  bn_backward_impl(d, out_diff, od_stride, xhat, xhat_stride, const_cast<float *>(scale), nullptr, inv_std, dscale, dshift, momentum, in_diff,
                   id_stride, act_y, act_stride, false, 0.0f, in, mean);
}
// backward + the component's own Update (scale -= lr*dscale, shift -= lr*dshift) in the statistics finalize
void aslp_bn_backward_step(MatrixDim d, const float *out_diff, int od_stride, float *xhat, int xhat_stride, float *scale, float *shift,
                           const float *inv_std, float *dscale, float *dshift, float momentum, float learn_rate, float *in_diff, int id_stride,
                           const float *act_y, int act_stride, const float *in, const float *mean) {
  bn_backward_impl(d, out_diff, od_stride, xhat, xhat_stride, scale, shift, inv_std, dscale, dshift, momentum, in_diff, id_stride, act_y,
                   act_stride, true, learn_rate, in, mean);
}
void aslp_bn_backward_step_p(MatrixDim d, const float *out_diff, int od_stride, float *xhat, int xhat_stride, float *scale, float *shift,
                             const float *inv_std, float *dscale, float *dshift, float momentum, float learn_rate, float *in_diff, int id_stride,
                             const float *act_y, int act_stride, const float *in, const float *mean, aslp_planes_out *diff_out) {
  bn_backward_impl(d, out_diff, od_stride, xhat, xhat_stride, scale, shift, inv_std, dscale, dshift, momentum, in_diff, id_stride, act_y,
                   act_stride, true, learn_rate, in, mean, diff_out);
}
// 1: a [rows x cols] batch is served by the single-launch panel kernels (given 16-byte aligned operands), which need no
// normalised copy of the input: pass xhat = NULL to the forward and backward entry points and save its 8.4 MB each way
int aslp_bn_panel_supported(int rows, int cols) { return bn_panel_shape(rows, cols) != 0 ? 1 : 0; }
// the choice aslp_bn_forward_act / bn_backward_impl make for 16-byte aligned operands, without a launch (tests name their instantiation by it)
int aslp_bn_path(int rows, int cols, int *q, int *slots) {
  const BnPath bp = bn_path_for(rows, cols, rows > 0 && cols > 0);
  if (q) *q = bp.q;
  if (slots) *slots = bp.slots;
  return bp.path;
}
void aslp_bn_backward(const float *in, MatrixDim d, const float *out_diff, int od_stride, float *xhat, int xhat_stride, const float *scale,
                      const float *mean, const float *inv_std, float *dscale, float *dshift, float momentum, float *in_diff, int id_stride) {
  aslp_bn_backward_act(in, d, out_diff, od_stride, xhat, xhat_stride, scale, mean, inv_std, dscale, dshift, momentum, in_diff, id_stride, nullptr,
                       0);
}

static bool xent_eval_impl(const float *net_out, MatrixDim d, const float *tgt, int tgt_stride, const int32_cuda *labels,
                           const float *frame_weights, float *diff, int diff_stride, double *stats_dev, bool softmax, float *y_out, int y_stride,
                           const aslp_planes_out *diff_planes = nullptr, double *rowstats_out = nullptr) {
  if (d.rows <= 0 || d.cols <= 0) return false;
  if (!tgt && !labels) { set_error("aslp_xent_eval: need dense targets or labels"); return false; }
  S16Out po = {nullptr, nullptr, 0, nullptr, nullptr};
  bool planes_written = false;
  // rowstats_out: the caller keeps the per-row statistics and adds them to its accumulators later (aslp_xent_sum_rowstats)
  double *rowstats = rowstats_out ? rowstats_out : static_cast<double *>(scratch(kScratchReduce, sizeof(double) * 5 * (size_t)d.rows));
  if (!rowstats) return false;
  int g = d.rows > kMaxGrid * 2 ? kMaxGrid * 2 : d.rows;
  if (d.cols > 256 * kXentPerThread) {   // wider than the register-cached kernels hold: the streaming kernel (the reference has no limit)
    if (softmax) { set_error("aslp_softmax_xent_eval: unsupported number of classes"); return false; }
    if (tgt) hipLaunchKernelGGL((xent_rows_wide_kernel<true>), dim3(g), dim3(256), 0, cur_stream(), net_out, d.stride, tgt, tgt_stride, labels, frame_weights,
                                diff, diff_stride, d.rows, d.cols, rowstats);
    else hipLaunchKernelGGL((xent_rows_wide_kernel<false>), dim3(g), dim3(256), 0, cur_stream(), net_out, d.stride, tgt, tgt_stride, labels, frame_weights,
                            diff, diff_stride, d.rows, d.cols, rowstats);
    if (!rowstats_out) hipLaunchKernelGGL(xent_finalize_kernel, dim3(1), dim3(256), 0, cur_stream(), rowstats, d.rows, stats_dev);
    check_launch("xent_eval");
    return false;
  }
  // elements cached per thread: the smallest of 4 / 8 / 16 / 32 that covers the row (the loops are fully unrolled: a row of
  // 3000 classes runs 16 slots per thread instead of 32 predicated ones)
  const int per = (d.cols + 255) / 256;
  if (diff_planes && diff_planes->hi && diff_planes->slot && !tgt && diff_planes->ld >= d.cols) {   // the row kernel, label targets
    po = S16Out{static_cast<h16 *>(diff_planes->hi), static_cast<h16 *>(diff_planes->lo), diff_planes->ld, diff_planes->slot, nullptr};
    planes_written = true;
  }
  // 16-byte accesses under softmax_rows_kernel's rule (same map: folding the Softmax into the loss changes no bit), every array's rows aligned
  const bool vec = softmax_rows_vec_ok(d.cols) && (d.stride & 3) == 0 && aligned16(net_out) && (diff_stride & 3) == 0 && aligned16(diff) &&
                   (!tgt || ((tgt_stride & 3) == 0 && aligned16(tgt))) && (!y_out || ((y_stride & 3) == 0 && aligned16(y_out))) &&
                   (!po.hi || ((po.ld & 3) == 0 && aligned16(po.hi) && aligned16(po.lo)));
#define XENT_LAUNCH_P(DENSE, SM, P)                                                                                                       \
  do {                                                                                                                                    \
    if (vec) hipLaunchKernelGGL((xent_rows_kernel<DENSE, SM, P, true>), dim3(g), dim3(256), 0, cur_stream(), net_out, d.stride, tgt, tgt_stride, labels, \
                                frame_weights, diff, diff_stride, d.rows, d.cols, rowstats, y_out, y_stride, po, nullptr);              \
    else hipLaunchKernelGGL((xent_rows_kernel<DENSE, SM, P>), dim3(g), dim3(256), 0, cur_stream(), net_out, d.stride, tgt, tgt_stride, labels, \
                            frame_weights, diff, diff_stride, d.rows, d.cols, rowstats, y_out, y_stride, po, nullptr);                  \
  } while (0)
#define XENT_LAUNCH(DENSE, SM)                                        \
  do {                                                                \
    if (per <= 4) XENT_LAUNCH_P(DENSE, SM, 4);                        \
    else if (per <= 8) XENT_LAUNCH_P(DENSE, SM, 8);                   \
    else if (per <= 16) XENT_LAUNCH_P(DENSE, SM, 16);                 \
    else XENT_LAUNCH_P(DENSE, SM, 32);                                \
  } while (0)
  if (tgt) { if (softmax) XENT_LAUNCH(true, true); else XENT_LAUNCH(true, false); }
  else { if (softmax) XENT_LAUNCH(false, true); else XENT_LAUNCH(false, false); }
#undef XENT_LAUNCH
#undef XENT_LAUNCH_P
  // (folding this sum into the rows' launch behind a ticket was measured: 54 us instead of 14 -- the device-scope release in front of the
  //  ticket makes every one of the 1024 workgroups write the L2 back, 12 MB of diff included)
  if (!rowstats_out) hipLaunchKernelGGL(xent_finalize_kernel, dim3(1), dim3(256), 0, cur_stream(), rowstats, d.rows, stats_dev);
  check_launch("xent_eval");
  return planes_written;
}

void aslp_xent_eval(const float *net_out, MatrixDim d, const float *tgt, int tgt_stride, const int32_cuda *labels, const float *frame_weights,
                    float *diff, int diff_stride, double *stats_dev) {
  xent_eval_impl(net_out, d, tgt, tgt_stride, labels, frame_weights, diff, diff_stride, stats_dev, false, nullptr, 0);
}
int aslp_xent_eval_p(const float *net_out, MatrixDim d, const int32_cuda *labels, const float *frame_weights, float *diff, int diff_stride,
                     double *stats_dev, int softmax, const aslp_planes_out *diff_planes) {
  if (softmax && !aslp_softmax_xent_supported(d.cols)) { set_error("aslp_softmax_xent_eval: unsupported number of classes"); return 0; }
  return xent_eval_impl(net_out, d, nullptr, 0, labels, frame_weights, diff, diff_stride, stats_dev, softmax != 0, nullptr, 0, diff_planes) ? 1 : 0;
}
// dst (nullable) <- src and src's planes in one launch; 1 = done (planes_written set), 0 = not served: the caller copies and converts
int aslp_copy_mat_planes(float *dst, MatrixDim d, const float *src, int src_stride, aslp_planes_out *out) {
  if (out) { out->nparts = 0; out->planes_written = 0; }
  if (!out || !out->hi || !out->lo || !out->slot || d.rows <= 0 || d.cols <= 0 || out->ld < d.cols) return 0;
  CoopConvJob job = {src, src_stride, dst, d.stride, S16View{static_cast<h16 *>(out->hi), static_cast<h16 *>(out->lo), out->ld, d.rows, d.cols,
                                                              const_cast<unsigned *>(out->slot)}, nullptr, 0};
  if (!coop_convert_launch(&job, 1)) return 0;
  out->planes_written = 1;
  return 1;
}
void aslp_coop_convert(int on) { g_coop_convert_on = on != 0; }
int aslp_xent_eval_rows(const float *net_out, MatrixDim d, const int32_cuda *labels, const float *frame_weights, float *diff, int diff_stride,
                        double *rowstats_out, int softmax, const aslp_planes_out *diff_planes) {
  if (!rowstats_out) { set_error("aslp_xent_eval_rows: no room for the per-row statistics"); return 0; }
  if (softmax && !aslp_softmax_xent_supported(d.cols)) { set_error("aslp_softmax_xent_eval: unsupported number of classes"); return 0; }
  return xent_eval_impl(net_out, d, nullptr, 0, labels, frame_weights, diff, diff_stride, nullptr, softmax != 0, nullptr, 0, diff_planes, rowstats_out) ? 1 : 0;
}
void aslp_xent_sum_rowstats(const double *rowstats, int rows, int batches, double *stats_dev) {
  if (rows <= 0 || batches <= 0) return;
  double *sums = static_cast<double *>(scratch(kScratchReduce, sizeof(double) * 5 * (size_t)batches));
  if (!sums) return;
  hipLaunchKernelGGL(xent_batch_sums_kernel, dim3(batches), dim3(256), 0, cur_stream(), rowstats, rows, sums);
  hipLaunchKernelGGL(xent_apply_kernel, dim3(1), dim3(64), 0, cur_stream(), sums, batches, stats_dev);
  check_launch("xent_sum_rowstats");
}
// Softmax + Xent::Eval in one pass over the activations in front of the Softmax; only rows of 513..8192 classes (the
// range where cudaF_softmax_reduce uses the same 256-lane row layout, so the posteriors are bit-identical)
int aslp_softmax_xent_supported(int cols) { return cols > 512 && cols <= 256 * kXentPerThread; }
void aslp_softmax_xent_eval(const float *acts, MatrixDim d, const float *tgt, int tgt_stride, const int32_cuda *labels,
                            const float *frame_weights, float *diff, int diff_stride, double *stats_dev, float *post_out, int post_stride) {
  if (!aslp_softmax_xent_supported(d.cols)) { set_error("aslp_softmax_xent_eval: unsupported number of classes"); return; }
  xent_eval_impl(acts, d, tgt, tgt_stride, labels, frame_weights, diff, diff_stride, stats_dev, true, post_out, post_stride);
}

// Xent on CSR targets (xent_rows_kernel<true, *, *, *, true>): the rung and the access path are chosen as xent_eval_impl chooses them for the
// dense matrix the entries stand for -- minus the target matrix' alignment, there being none.  false = refused, nothing launched.
int aslp_xent_sparse_supported(int cols, int softmax) {
  return softmax ? aslp_softmax_xent_supported(cols) : (cols >= 1 && cols <= 256 * kXentPerThread ? 1 : 0);
}
static bool xent_sparse_impl(const char *who, const float *in, MatrixDim d, const int32_cuda *row_begin, const int32_cuda *tgt_col, const float *tgt_w,
                             const float *frame_weights, float *diff, int diff_stride, double *stats_dev, double *rowstats_out, bool softmax,
                             float *y_out, int y_stride) {
  auto refuse = [&](const char *what) { set_error(std::string(who) + ": " + what); return false; };
  if (!in || !row_begin || !tgt_col || !tgt_w || !frame_weights || !diff || (!stats_dev && !rowstats_out)) return refuse("null argument");
  if (d.rows <= 0 || d.cols <= 0 || d.stride < d.cols || diff_stride < d.cols || (y_out && y_stride < d.cols))
    return refuse("sizes must be positive and no stride smaller than the number of columns");
  if (!aslp_xent_sparse_supported(d.cols, softmax ? 1 : 0)) return refuse("unsupported number of classes");
  if (!softmax) y_out = nullptr;   // (the posteriors are the input)
  double *rowstats = rowstats_out ? rowstats_out : static_cast<double *>(scratch(kScratchReduce, sizeof(double) * 5 * (size_t)d.rows));
  if (!rowstats) return false;
  const int g = d.rows > kMaxGrid * 2 ? kMaxGrid * 2 : d.rows;
  const int per = (d.cols + 255) / 256;
  const S16Out po = {nullptr, nullptr, 0, nullptr, nullptr};
  const bool vec = softmax_rows_vec_ok(d.cols) && (d.stride & 3) == 0 && aligned16(in) && (diff_stride & 3) == 0 && aligned16(diff) &&
                   (!y_out || ((y_stride & 3) == 0 && aligned16(y_out)));
#define XENT_SPARSE_P(SM, P)                                                                                                                      \
  do {                                                                                                                                            \
    if (vec) hipLaunchKernelGGL((xent_rows_kernel<true, SM, P, true, true>), dim3(g), dim3(256), 0, cur_stream(), in, d.stride, tgt_w, 0, tgt_col, \
                                frame_weights, diff, diff_stride, d.rows, d.cols, rowstats, y_out, y_stride, po, row_begin);                      \
    else hipLaunchKernelGGL((xent_rows_kernel<true, SM, P, false, true>), dim3(g), dim3(256), 0, cur_stream(), in, d.stride, tgt_w, 0, tgt_col,   \
                            frame_weights, diff, diff_stride, d.rows, d.cols, rowstats, y_out, y_stride, po, row_begin);                          \
  } while (0)
#define XENT_SPARSE(SM)                                \
  do {                                                 \
    if (per <= 4) XENT_SPARSE_P(SM, 4);                \
    else if (per <= 8) XENT_SPARSE_P(SM, 8);           \
    else if (per <= 16) XENT_SPARSE_P(SM, 16);         \
    else XENT_SPARSE_P(SM, 32);                        \
  } while (0)
  if (softmax) XENT_SPARSE(true); else XENT_SPARSE(false);
#undef XENT_SPARSE
#undef XENT_SPARSE_P
  if (!rowstats_out) hipLaunchKernelGGL(xent_finalize_kernel, dim3(1), dim3(256), 0, cur_stream(), rowstats, d.rows, stats_dev);
  check_launch(who);
  return true;
}
int aslp_xent_sparse_eval(const float *in, MatrixDim d, const int32_cuda *row_begin, const int32_cuda *tgt_col, const float *tgt_w,
                          const float *frame_weights, float *diff, int diff_stride, double *stats_dev, int softmax, float *post_out, int post_stride) {
  if (!stats_dev) { set_error("aslp_xent_sparse_eval: null argument"); return 0; }
  return xent_sparse_impl("aslp_xent_sparse_eval", in, d, row_begin, tgt_col, tgt_w, frame_weights, diff, diff_stride, stats_dev, nullptr, softmax != 0,
                          post_out, post_stride) ? 1 : 0;
}
int aslp_xent_sparse_eval_rows(const float *in, MatrixDim d, const int32_cuda *row_begin, const int32_cuda *tgt_col, const float *tgt_w,
                               const float *frame_weights, float *diff, int diff_stride, double *rowstats_out, int softmax, float *post_out,
                               int post_stride) {
  if (!rowstats_out) { set_error("aslp_xent_sparse_eval_rows: no room for the per-row statistics"); return 0; }
  return xent_sparse_impl("aslp_xent_sparse_eval_rows", in, d, row_begin, tgt_col, tgt_w, frame_weights, diff, diff_stride, nullptr, rowstats_out,
                          softmax != 0, post_out, post_stride) ? 1 : 0;
}

// Mse::Eval in one launch (mse_rows_kernel above).  16-byte accesses where all three matrices allow them, one column per access elsewhere
// (a MultiTask window at an odd column of a wider matrix).  0 = refused, nothing launched.
int aslp_mse_eval_w(const float *net_out, MatrixDim d, const float *tgt, int tgt_stride, const float *frame_weights, float scale, float *diff,
                    int diff_stride, double *row_loss, aslp_planes_out *diff_out, double *frames_out) {
  if (diff_out) { diff_out->nparts = 0; diff_out->planes_written = 0; }
  if (!net_out || !tgt || !frame_weights || !diff || !row_loss) { set_error("aslp_mse_eval: null argument"); return 0; }
  if (d.rows <= 0 || d.cols <= 0 || d.stride < d.cols || tgt_stride < d.cols || diff_stride < d.cols) {
    set_error("aslp_mse_eval: sizes must be positive and no stride smaller than the number of columns");
    return 0;
  }
  const bool vec = aligned16(net_out) && aligned16(tgt) && aligned16(diff) && (d.stride & 3) == 0 && (tgt_stride & 3) == 0 && (diff_stride & 3) == 0;
  float *parts = diff_out ? diff_out->parts : nullptr;
  const int g = std::min((d.rows + kPanelWaves - 1) / kPanelWaves, kS16ConvParts);
  const dim3 grid(g + (frames_out ? 1 : 0));
  if (vec) hipLaunchKernelGGL((mse_rows_kernel<true>), grid, dim3(kPanelThreads), 0, cur_stream(), net_out, d.stride, tgt, tgt_stride, frame_weights, scale,
                              diff, diff_stride, d.rows, d.cols, row_loss, parts, frames_out);
  else hipLaunchKernelGGL((mse_rows_kernel<false>), grid, dim3(kPanelThreads), 0, cur_stream(), net_out, d.stride, tgt, tgt_stride, frame_weights, scale,
                          diff, diff_stride, d.rows, d.cols, row_loss, parts, frames_out);
  check_launch("mse_eval");
  if (parts) diff_out->nparts = g;
  return 1;
}
int aslp_mse_eval(const float *net_out, MatrixDim d, const float *tgt, int tgt_stride, const float *frame_weights, float scale, float *diff,
                  int diff_stride, double *row_loss, aslp_planes_out *diff_out) {
  return aslp_mse_eval_w(net_out, d, tgt, tgt_stride, frame_weights, scale, diff, diff_stride, row_loss, diff_out, nullptr);
}
void aslp_mse_batch_sums(const double *pending, int rows, int batches, double *sums) {
  if (!pending || !sums || rows <= 0 || batches <= 0) return;
  hipLaunchKernelGGL(mse_batch_sums_kernel, dim3(batches), dim3(256), 0, cur_stream(), pending, rows, sums);
  check_launch("mse_batch_sums");
}

// Xent over up to 16 column blocks of one matrix in one launch (xent_blocks_kernel above).  0 = refused, nothing launched.
int aslp_xent_blocks_supported(int block_cols) { return block_cols >= 1 && block_cols <= 256 * kXentPerThread; }
int aslp_xent_blocks_eval(const float *in, MatrixDim d, const aslp_xent_block *blocks, int n_blocks, const int32_cuda *labels,
                          const float *frame_weights, float *diff, int diff_stride, int softmax, int mask, float *post_out, int post_stride,
                          aslp_planes_out *diff_out) {
  if (diff_out) { diff_out->nparts = 0; diff_out->planes_written = 0; }
  if (!in || !blocks || !labels || !frame_weights || !diff) { set_error("aslp_xent_blocks_eval: null argument"); return 0; }
  if (d.rows <= 0 || d.cols <= 0 || d.stride < d.cols || diff_stride < d.cols || (post_out && post_stride < d.cols)) {
    set_error("aslp_xent_blocks_eval: sizes must be positive and no stride smaller than the number of columns");
    return 0;
  }
  if (n_blocks <= 0 || n_blocks > kXbMaxBlocks) { set_error("aslp_xent_blocks_eval: 1 .. 16 blocks"); return 0; }
  XbArgs a;
  a.n = n_blocks;
  a.vec = a.dvec = 0u;
  int widest = 0;
  for (int b = 0; b < n_blocks; b++) {
    const aslp_xent_block &k = blocks[b];
    if (!k.rowstats) { set_error("aslp_xent_blocks_eval: a block without room for its row statistics"); return 0; }
    if (!aslp_xent_blocks_supported(k.cols)) { set_error("aslp_xent_blocks_eval: a block must be 1 .. 8192 columns wide"); return 0; }
    if (k.offset < 0 || k.offset > d.cols - k.cols) { set_error("aslp_xent_blocks_eval: a block outside the matrix"); return 0; }
    for (int o = 0; o < b; o++)
      if (k.offset < blocks[o].offset + blocks[o].cols && blocks[o].offset < k.offset + k.cols) {
        set_error("aslp_xent_blocks_eval: overlapping blocks");
        return 0;
      }
    a.off[b] = k.offset; a.cols[b] = k.cols; a.weight[b] = k.weight; a.rs[b] = k.rowstats;
    if (k.cols > kXbWaveCols) {
      widest = std::max(widest, k.cols);
      // launch_softmax' rule for the window: its rows and the posteriors' on 16-byte boundaries
      const bool vec = softmax_rows_vec_ok(k.cols) && (d.stride & 3) == 0 && aligned16(in + k.offset) &&
                       (!post_out || ((post_stride & 3) == 0 && aligned16(post_out + k.offset)));
      if (vec) a.vec |= 1u << b;
      if (vec && (diff_stride & 3) == 0 && aligned16(diff + k.offset)) a.dvec |= 1u << b;
    }
  }
  float *parts = diff_out ? diff_out->parts : nullptr;
  const int g = std::min(d.rows, kS16ConvParts);
  const int per = (widest + 255) / 256;
#define XB_LAUNCH(P)                                                                                                                          \
  hipLaunchKernelGGL((xent_blocks_kernel<P>), dim3(g), dim3(256), 0, cur_stream(), in, d.stride, a, labels, frame_weights, diff, diff_stride, \
                     d.rows, softmax, mask, post_out, post_stride, parts)
  if (per <= 4) XB_LAUNCH(4);
  else if (per <= 8) XB_LAUNCH(8);
  else if (per <= 16) XB_LAUNCH(16);
  else XB_LAUNCH(32);
#undef XB_LAUNCH
  check_launch("xent_blocks_eval");
  if (parts) diff_out->nparts = g;
  return 1;
}

}  // extern "C"
