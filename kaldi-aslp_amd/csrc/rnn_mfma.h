// rnn_mfma.h -- the skinny-product building blocks shared by the fused recurrent step kernels (rnn_fused.hip,
// gru_fused.hip): a 32 x 32 output tile (32 streams x 32 gate columns), K split over the 4 waves of a workgroup, both
// operands K-contiguous in global memory, partial tiles combined through LDS in wave order.
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

}  // namespace
}  // namespace aslp
