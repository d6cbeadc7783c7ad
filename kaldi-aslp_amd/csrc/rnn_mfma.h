// rnn_mfma.h -- the skinny products of the fused recurrent step kernels (rnn_fused.hip, gru_fused.hip), each written once:
// a 32 x 32 output tile (32 streams x 32 gate columns), K split into contiguous slices (one per wave, or per K-part x
// wave), both operands K-contiguous in global memory, partial tiles combined through LDS in wave order.
//   product_f32                  one slice on v_mfma_f32_32x32x2_f32 into the wave's partial tile
//   product_h / product_t_h      the same on v_mfma_f32_32x32x16_f16 with operands as fp16 pieces (forward / transposed backward); called by
//                                the GRU kernels, held inline by lstm_step_fwd_h / lstm_step_bwd_gemm_h (see there): change both
//   tile_sum                     the waves' partial tiles, added in wave order
//   planes_ok                    what a launch of product_h / product_t_h needs of the planes it reads (host)
#pragma once
#include "common.h"
#include "split16.h"

namespace aslp {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int kPad = 33;  // LDS row pitch of a 32 x 32 partial tile

__device__ __forceinline__ float dsigm(float y, float d) { return d * y * (1.0f - y); }
__device__ __forceinline__ float dtanh(float y, float d) { return d * (1.0f - y * y); }

// acc += A[32 x K-slice] * B[32 x K-slice]^T over the 8-wide K-chunks [qbegin, qend): a CONTIGUOUS slice per wave,
// so every 128-B line of an operand row is pulled by exactly one wave.
// arow / brow: this lane's operand rows (lane & 31), K-contiguous, 16-B aligned; K % 4 == 0.
template <int U = 8>
__device__ __forceinline__ void mfma_k_slices(f32x16 &acc, const float *__restrict__ arow, const float *__restrict__ brow, int K, int qbegin,
                                              int qend, int h) {
  // U: 8-wide K-chunks in flight
  for (int q0 = qbegin; q0 < qend; q0 += U) {
    float4 a[U], b[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int k = 8 * (q0 + u) + 4 * h;
      const bool ok = (q0 + u) < qend && k < K;
      const int kk = ok ? k : 0;
      a[u] = *reinterpret_cast<const float4 *>(arow + kk);
      b[u] = *reinterpret_cast<const float4 *>(brow + kk);
      if (!ok) { a[u] = make_float4(0.f, 0.f, 0.f, 0.f); b[u] = make_float4(0.f, 0.f, 0.f, 0.f); }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].x, b[u].x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].y, b[u].y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].z, b[u].z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].w, b[u].w, acc, 0, 0, 0);
    }
  }
}

// C/D layout of v_mfma_f32_32x32x2f32: element e of lane l is row (e&3) + 8*(e>>2) + 4*(l>>5), column l&31
__device__ __forceinline__ void store_tile(float *tile, const f32x16 &acc, int lane) {
  const int n = lane & 31, h = lane >> 5;
#pragma unroll
  for (int e = 0; e < 16; e++) tile[((e & 3) + 8 * (e >> 2) + 4 * h) * kPad + n] = acc[e];
}

// the transposed tile (the product was taken as B A^T: rows of the accumulator are tile columns): tile[column of acc][row of acc]
__device__ __forceinline__ void store_tile_t(float *tile, const f32x16 &acc, int lane) {
  const int n = lane & 31, h = lane >> 5;
#pragma unroll
  for (int e = 0; e < 16; e++) tile[n * kPad + (e & 3) + 8 * (e >> 2) + 4 * h] = acc[e];
}

// One K slice -- `part` of `nparts` contiguous runs of 8-wide K-chunks -- of a product into this wave's partial tile; !on stores zeros.
template <int U = 8>
__device__ __forceinline__ void product_f32(float *tile, const float *arow, const float *brow, int K, int part, int nparts,
                                            int lane, bool on) {
  f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int nch = (K + 7) / 8, per = (nch + nparts - 1) / nparts;
  if (on) mfma_k_slices<U>(acc, arow, brow, K, part * per, min(nch, (part + 1) * per), lane >> 5);
  store_tile(tile, acc, lane);
}

// element (row, col) of the product: the NW waves' partial tiles, added in wave order (deterministic)
template <int NW = 4>
__device__ __forceinline__ float tile_sum(const float (*red)[32 * kPad], int row, int col) {
  float acc = red[0][row * kPad + col];
#pragma unroll
  for (int w = 1; w < NW; w++) acc += red[w][row * kPad + col];
  return acc;
}

// ---- the same products on v_mfma_f32_32x32x16_f16 with operands as fp16 pieces (csrc/split16.h: x s = hi + 2^-11 lo') ----------------
// Operand map of the instruction: lane l holds A[row l & 31][k = 8 (l >> 5) + j] and B[k = 8 (l >> 5) + j][column l & 31], j = 0..7; C/D as above.
// NP pieces of 8 consecutive fp32 values behind the power-of-two scale s
template <int NP>
__device__ __forceinline__ void split8(const float4 &u, const float4 &v, float s, half8 &hi, half8 &lo) {
  const float x[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const float y = x[i] * s;
    const h16 hh = (h16)y;
    hi[i] = hh;
    if (NP == 2) lo[i] = (h16)((y - (float)hh) * 2048.f);
  }
}

// One run of up to U 16-wide k steps [q0, min(q0 + U, qend)) of a 32 x 32 tile: the fp16 counterpart of one round of mfma_k_slices.
//   frow        this lane's row (lane & 31) of the fp32 operand, K-contiguous, 16-B aligned, K % 4 == 0 valid columns: split into NP pieces
//               as it is loaded; columns >= K are never addressed and enter as zeros
//   phi / plo   this lane's row of the other operand's planes; read up to K rounded up to 16 (the planes' padding: zeros)
//   SCALED      the fp32 operand sits behind a power-of-two scale formed here from the largest finite |value| of this lane's row within the
//               run (both lane halves; an all-zero run: scale 1); *inv_s returns its inverse.  Not SCALED: scale 1 (|value| <= 1)
//   F32_IS_B    the fp32 operand supplies the tile's columns (B), the planes its rows (A); else the other way round
// acc_hh += hi hi; NP == 2: acc_x += hi lo' + lo' hi (the caller adds 2^-11 acc_x; lo' lo' is dropped).  Fixed order: k step by k step.
template <int NP, int U, bool SCALED, bool F32_IS_B>
__device__ __forceinline__ void mfma_run_h(f32x16 &acc_hh, f32x16 &acc_x, const float *__restrict__ frow, int K, const h16 *__restrict__ phi,
                                           const h16 *__restrict__ plo, int q0, int qend, int h, float *inv_s) {
  float4 x0[U], x1[U];
  half8 whi[U], wlo[U];
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int k = 16 * (q0 + u) + 8 * h;
    const bool ok = (q0 + u) < qend, ok0 = ok && k < K, ok1 = ok && k + 4 < K;
    whi[u] = *reinterpret_cast<const half8 *>(phi + (ok ? k : 0));
    if (NP == 2) wlo[u] = *reinterpret_cast<const half8 *>(plo + (ok ? k : 0));
    x0[u] = *reinterpret_cast<const float4 *>(frow + (ok0 ? k : 0));
    x1[u] = *reinterpret_cast<const float4 *>(frow + (ok1 ? k + 4 : 0));
    if (!ok0) x0[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!ok1) x1[u] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float s = 1.0f;
  if (SCALED) {
    float m = 0.f;
#pragma unroll
    for (int u = 0; u < U; u++) m = s16_absmax4(s16_absmax4(m, x0[u]), x1[u]);
    m = fmaxf(m, __shfl_xor(m, 32));
    const int up = s16_exponent(__float_as_uint(m));
    s = ldexpf(1.0f, up);
    *inv_s = ldexpf(1.0f, -up);
  }
#pragma unroll
  for (int u = 0; u < U; u++) {
    half8 fhi, flo;
    split8<NP>(x0[u], x1[u], s, fhi, flo);
    if (F32_IS_B) {
      acc_hh = __builtin_amdgcn_mfma_f32_32x32x16_f16(whi[u], fhi, acc_hh, 0, 0, 0);
      if (NP == 2) {
        acc_x = __builtin_amdgcn_mfma_f32_32x32x16_f16(wlo[u], fhi, acc_x, 0, 0, 0);
        acc_x = __builtin_amdgcn_mfma_f32_32x32x16_f16(whi[u], flo, acc_x, 0, 0, 0);
      }
    } else {
      acc_hh = __builtin_amdgcn_mfma_f32_32x32x16_f16(fhi, whi[u], acc_hh, 0, 0, 0);
      if (NP == 2) {
        acc_x = __builtin_amdgcn_mfma_f32_32x32x16_f16(fhi, wlo[u], acc_x, 0, 0, 0);
        acc_x = __builtin_amdgcn_mfma_f32_32x32x16_f16(flo, whi[u], acc_x, 0, 0, 0);
      }
    }
  }
}

// 16-wide k steps in flight per wave: one run of mfma_run_h, and the extent of one backward scale (128 consecutive k)
constexpr int kRunH = 8;

// One K slice -- `part` of `nparts` contiguous runs of 16-wide k steps -- of a forward product into this wave's partial tile: frow (this
// lane's stream row of m(t-1) / h(t-1) / g(t), |value| <= 1) is split into NP pieces as it is loaded, without a scale; phi / plo are this
// lane's gate-column row of the weight planes, scaled by the bound in *slot.  The k tail (K % 16) reads the planes' zero padding.
template <int NP>
__device__ __forceinline__ void product_h(float *tile, const float *frow, int K, const h16 *phi, const h16 *plo,
                                          const unsigned *slot, int part, int nparts, int lane, bool on) {
  const float inv_w = ldexpf(1.0f, -s16_exponent(*slot));
  f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, acx = acc;
  const int nst = (K + 15) / 16, per = (nst + nparts - 1) / nparts, qend = min(nst, (part + 1) * per);
  if (on)
    for (int q0 = part * per; q0 < qend; q0 += kRunH) mfma_run_h<NP, kRunH, false, false>(acc, acx, frow, K, phi, plo, q0, qend, lane >> 5, nullptr);
  if (NP == 2) acc += acx * (1.0f / 2048.f);
  acc *= inv_w;
  store_tile(tile, acc, lane);
}

// The same for a backward product, taken transposed: the planes' rows (cells of W^T) are the A operand and drow (this lane's stream row of
// dGATES(t+1) / [d_z | d_r](t+1) / d_m(t)) is B, so a stream is a lane's COLUMN of the accumulator and its power-of-two scale -- one per
// stream row and run of kRunH k steps, runs counted from the start of the slice, formed from the run's largest finite |value| as it is
// loaded -- is a per-lane factor, taken out again before the run joins the slice's fp32 sum.  An all-zero run takes scale 1 and adds an
// exact zero.
template <int NP>
__device__ __forceinline__ void product_t_h(float *tile, const float *drow, int K, const h16 *phi, const h16 *plo,
                                            const unsigned *slot, int part, int nparts, int lane, bool on) {
  const float inv_w = ldexpf(1.0f, -s16_exponent(*slot));
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  f32x16 tot = zero;
  const int nst = (K + 15) / 16, per = (nst + nparts - 1) / nparts, qend = min(nst, (part + 1) * per);
  if (on)
    for (int q0 = part * per; q0 < qend; q0 += kRunH) {
      f32x16 acc = zero, acx = zero;
      float inv_s = 1.0f;
      mfma_run_h<NP, kRunH, true, true>(acc, acx, drow, K, phi, plo, q0, qend, lane >> 5, &inv_s);
      if (NP == 2) acc += acx * (1.0f / 2048.f);
      tot += acc * inv_s;
    }
  tot *= inv_w;
  store_tile_t(tile, tot, lane);
}

// the planes such a launch reads: hi (lo with two pieces) 16-byte aligned, the slot present, and K rounded up to 16 halves inside a plane row
inline bool planes_ok(const void *hi, const void *lo, const unsigned *slot, int ldp, int K, int np) {
  return hi != nullptr && aligned16(hi) && slot != nullptr && (np == 1 || (lo != nullptr && aligned16(lo))) && (ldp & 7) == 0 && ldp >= (K + 15) / 16 * 16;
}

}  // namespace
}  // namespace aslp
