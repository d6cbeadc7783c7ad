// gemm_s16_kernels.h -- device side of the split-fp16 products: what the three kernels share behind the K loop (weight bound, s16_finish,
// column sums, s16_pick) and the kernels themselves (gemm_s16_glds, gemm_s16_ks128, gemm_s16_pc).  An implementation header of
// gemm_split16.hip, which explains the method and holds the plane format's conversion kernels, the launchers and the tile choice;
// devtools/micro/s16_ablate.hip and s16_pc.hip get it through that file.
//
// The K-loop parts (DMA descriptors, fragment offsets, read_unit, mma_unit) are still written out per kernel: factored into shared
// __forceinline__ templates they came out of this compiler with other register counts and SGPR spills on 21 of the 39 instantiations
// (e.g. gemm_s16_glds<64,128,2,2,3,false,false,0,true,2>: 252 -> 254 VGPRs, 16 -> 29 spilled SGPRs), so they stay as they are until
// that can be done with identical code.  A fix to a clamp or a swizzle has to be made in all three.
#pragma once
#include "gemm_common.h"
#include "split16.h"

#pragma clang diagnostic ignored "-Winline-asm"  // the DMA asm clobbers m0 on purpose

namespace aslp {
namespace {

constexpr int BKH = 64;       // halves per K tile
constexpr int KH = BKH / 16;  // instruction k steps per tile
typedef __attribute__((address_space(3))) char lds_char;
typedef short short4v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) short4v lds_short4;

// KS image: XOR of the 64-byte column-group index of k row `krow` (BR halves per row)
template <int BR>
__device__ __forceinline__ int ks_swizzle(int krow) { return BR == 64 ? ((krow >> 1) & 1) : BR == 128 ? (krow & 3) : 0; }

// ---- shared by the product kernels ------------------------------------------------------------------------------------------------
// (EXTRA) the bound of the weights after the fused step: |W + w_alpha C| <= max |W| + |w_alpha| (|alpha| K max|a| max|b| + |beta| max |C_old|),
// the maxima from the previous step's per-workgroup partials.  Every wave forms it; workgroup 0 stores it for the planes' readers.
__device__ __forceinline__ float s16_weight_bound(const GemmArgs &g, const S16View &va, const S16View &vb, int lane) {
  if (g.ep.bound_w_parts == nullptr) return 0.f;   // uniform
  // (four independent loads per array and pass: a dependent load per element here once cost every weight-gradient launch 50 us)
  float mw = 0.f, mc = 0.f;
  const int n = g.ep.bound_n;
  const float *wp = g.ep.bound_w_parts, *cp = g.ep.bound_c_parts;
  for (int i = lane; i < n; i += 256) {
    const int i1 = i + 64, i2 = i + 128, i3 = i + 192;
    const float a0 = wp[i], a1 = i1 < n ? wp[i1] : 0.f, a2 = i2 < n ? wp[i2] : 0.f, a3 = i3 < n ? wp[i3] : 0.f;
    mw = fmaxf(fmaxf(mw, fmaxf(a0, a1)), fmaxf(a2, a3));
    if (cp != nullptr) {
      const float c0 = cp[i], c1 = i1 < n ? cp[i1] : 0.f, c2 = i2 < n ? cp[i2] : 0.f, c3 = i3 < n ? cp[i3] : 0.f;
      mc = fmaxf(fmaxf(mc, fmaxf(c0, c1)), fmaxf(c2, c3));
    }
  }
  mw = wave_max(mw);
  mc = wave_max(mc);
  float v = fabsf(g.alpha) * (float)g.K * __uint_as_float(*va.slot) * __uint_as_float(*vb.slot) + fabsf(g.beta) * mc;
  if (g.ep.clip > 0.f) v = fminf(v, g.ep.clip);
  const float w_bound = mw + fabsf(g.ep.w_alpha) * v;
  if (blockIdx.x == 0 && blockIdx.z == 0 && threadIdx.x == 0) *const_cast<unsigned *>(g.ep.planes.slot) = __float_as_uint(w_bound);
  return w_bound;
}

// Everything behind the K loop: join the two accumulators and undo the operand scales, the column sums of a reduction-major A
// (COLSUM), the column statistics, the epilogue (with the planes / maxima of its output when EXTRA).  (row0, col0): this wave's patch.
// NP = 1 (one-plane products): there is no cross-term accumulator to join.
template <int TM, int TN, int NW, bool EXTRA, bool COLSUM, int NP = 2>
__device__ __forceinline__ void s16_finish(const GemmArgs &g, const S16View &va, const S16View &vb, f32x16 (&acc)[TM][TN], const f32x16 (&accx)[TM][TN],
                                           const float (&asum)[TM], bool do_colsum, float w_bound, int row0, int col0, int lane, int wave, float *lds) {
  const int l31 = lane & 31, lh = lane >> 5;
  // 2^-(up_a + up_b) in two exact factors (either alone may leave fp32's range where their product with the accumulator does not)
  {
    const int e = -(s16_exponent(*va.slot) + s16_exponent(*vb.slot));
    const float s1 = ldexpf(1.f, e / 2), s2 = ldexpf(1.f, e - e / 2);
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
      for (int j = 0; j < TN; j++)
#pragma unroll
        for (int q = 0; q < 16; q++) {
          if constexpr (NP == 2) acc[i][j][q] = (fmaf(accx[i][j][q], 0x1p-11f, acc[i][j][q]) * s1) * s2;
          else acc[i][j][q] = (acc[i][j][q] * s1) * s2;
        }
  }
  if constexpr (COLSUM) {
    if (do_colsum) {
      const float inv_a = ldexpf(1.f, -s16_exponent(*va.slot));
#pragma unroll
      for (int i = 0; i < TM; i++) {
        const float s_all = (asum[i] + __shfl_xor(asum[i], 32, 64)) * inv_a;  // the two lane halves hold disjoint k subsets
        const int row = row0 + i * 32 + l31;
        if (lh == 0 && row < g.M) {
          float v = s_all;
          if (g.ep.colsum_beta != 0.0f) v += g.ep.colsum_beta * g.ep.colsum[row];
          g.ep.colsum[row] = v;
          if (g.ep.colsum_w) g.ep.colsum_w[row] += g.ep.colsum_w_alpha * v;
        }
      }
    }
  }
  if (g.ep.colstats != nullptr) gemm_colstats<TM, TN>(g, acc, row0, col0, l31, lh);  // uniform
  // planes of an output and per-workgroup maxima for the products that will read it (aslp_gemm_epilogue.planes / *_parts)
  EpiExtra xtra;
  if constexpr (EXTRA) {
    if (g.ep.planes_of != 0 && g.ep.planes.hi != nullptr)
      xtra.pscale = ldexpf(1.f, s16_exponent(g.ep.bound_w_parts != nullptr ? __float_as_uint(w_bound) : *g.ep.planes.slot));
  }
  if (g.wide_epilogue && gemm_epilogue_wide_ok(g)) {  // uniform
    __builtin_amdgcn_s_barrier();
    gemm_epilogue_wide<TM, TN>(g, acc, row0, col0, lane, lds + wave * 32 * kEpiPitch, xtra, EXTRA);
  } else {
    gemm_epilogue<TM, TN>(g, acc, row0, col0, l31, lh, xtra, false);   // (the host asks for planes / maxima only where the wide epilogue applies)
  }
  if (EXTRA && (g.ep.wmax_parts != nullptr || g.ep.cmax_parts != nullptr)) {   // one maximum per workgroup: the waves meet in LDS
    const float wmx = wave_max(xtra.wmax), cmx = wave_max(xtra.cmax);
    __builtin_amdgcn_s_barrier();   // every wave is done with its epilogue slice of the LDS
    if (lane == 0) { lds[2 * wave] = wmx; lds[2 * wave + 1] = cmx; }
    __syncthreads();
    if (threadIdx.x == 0) {
      float w = lds[0], c = lds[1];
#pragma unroll
      for (int q = 1; q < NW; q++) { w = fmaxf(w, lds[2 * q]); c = fmaxf(c, lds[2 * q + 1]); }
      const int idx = (int)blockIdx.z * (int)gridDim.x + (int)blockIdx.x;
      if (g.ep.wmax_parts) g.ep.wmax_parts[idx] = w;
      if (g.ep.cmax_parts) g.ep.cmax_parts[idx] = c;
    }
  }
  // ... and of |act_out| (amax_parts: an activation without a bound known before the launch).  Words of their own behind the 2 NW above,
  // which thread 0 may still be reading
  if (EXTRA && g.ep.amax_parts != nullptr) {   // (uniform)
    const float amx = wave_max(xtra.amax);
    __builtin_amdgcn_s_barrier();   // every wave is done with its epilogue slice of the LDS
    if (lane == 0) lds[2 * NW + wave] = amx;
    __syncthreads();
    if (threadIdx.x == 0) {
      float a = lds[2 * NW];
#pragma unroll
      for (int q = 1; q < NW; q++) a = fmaxf(a, lds[2 * NW + q]);
      g.ep.amax_parts[(int)blockIdx.z * (int)gridDim.x + (int)blockIdx.x] = a;
    }
  }
}
// column sums of a reduction-major A from the fragments a wave multiplies anyway: sum over the 8 k of a fragment of hi + 2^-11 lo'
__device__ __forceinline__ float s16_frag_sum(float sum, const half8 hi, const half8 lo) {
  typedef _Float16 half2v __attribute__((ext_vector_type(2)));
  const half2v one = {(h16)1.0f, (h16)1.0f}, eps = {(h16)0x1p-11f, (h16)0x1p-11f};
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const half2v hv = {hi[2 * q], hi[2 * q + 1]}, lv = {lo[2 * q], lo[2 * q + 1]};
    sum = __builtin_amdgcn_fdot2(hv, one, sum, false);     // fp32 accumulation of exact fp16 values
    sum = __builtin_amdgcn_fdot2(lv, eps, sum, false);
  }
  return sum;
}

// ---- the product ---------------------------------------------------------------------------------------------------------------
struct S16Operands { S16View a, b, a1, b1; int kp; };   // a1 / b1: second product of a pair (blockIdx.z == 1)
// one of two views, member by member: assigning a whole struct under a condition makes hipcc park both in scratch memory (88 bytes per
// lane and a private segment on every product kernel)
__device__ __forceinline__ S16View s16_pick(bool second, const S16View &x, const S16View &y) {
  S16View v;
  v.hi = second ? +y.hi : +x.hi;
  v.lo = second ? +y.lo : +x.lo;
  v.ld = second ? +y.ld : +x.ld;
  v.rows = second ? +y.rows : +x.rows;
  v.cols = second ? +y.cols : +x.cols;
  v.slot = second ? +y.slot : +x.slot;
  return v;
}

// ABL (devtools/micro/s16_ablate.hip only; 0 in the library): 1 = no MFMA, 2 = no DMA, 4 = no LDS reads -- wrong results, for timing
// EXTRA: the epilogue also leaves planes / maxima of its output (aslp_gemm_epilogue.planes, *_parts); a variant of its own because the
// extra epilogue state costs the 128 x 128 tile its last registers.
// NP: planes read per operand.  2 = hi and lo (everything above).  1 = the hi plane alone (aslp_gemm_operand_planes(1)): the operands are
// X16 = fp16(X 2^up) 2^-up, 11 significant bits, a stage is A_hi | B_hi, a k step is ONE matrix instruction into the one accumulator -- half
// the bytes through L2 -> LDS, half the LDS reads, a third of the matrix instructions; the pipeline, the images and the epilogue are the same.
template <int BM, int BN, int WGM, int WGN, int NS, bool A_KC, bool B_KC, int ABL = 0, bool EXTRA = false, int NP = 2>
__global__ void __launch_bounds__(64 * WGM * WGN)
    __attribute__((amdgpu_waves_per_eu(1, (NS * NP * (BM + BN) * 128 > 80 * 1024 && WGM * WGN <= 4) ? 1 : 2)))   // (LDS already limits those to one wave per SIMD: all 512 registers are theirs)
    gemm_s16_glds(GemmArgs g, S16Operands ops) {
  constexpr int NW = WGM * WGN;
  constexpr int WM = BM / WGM, WN = BN / WGN, TM = WM / 32, TN = WN / 32;
  // a stage, in bytes (every plane tile is 64 halves x BR rows whichever way it lies): A_hi | A_lo | B_hi | B_lo
  static_assert(NP == 1 || NP == 2, "one or two planes per operand");
  constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, STAGE = NP * (A_BYTES + B_BYTES);
  constexpr int SLOTS_A = BM / 8, SLOTS_B = BN / 8, SLOTS = NP * (SLOTS_A + SLOTS_B);   // 1-KiB DMA units per tile
  static_assert(SLOTS % NW == 0, "DMA units must divide over the waves");
  constexpr int G = SLOTS / NW;
  constexpr int D = NS - 1;
  constexpr int RA = A_KC ? 1 : 2, RB = B_KC ? 1 : 2;            // LDS reads per fragment and plane
  constexpr int NRH = NP * (TM * RA + TN * RB);                   // reads per instruction k step
  constexpr int NI = NP == 2 ? 3 : 1;                             // matrix instructions per k step and pair of fragments
  constexpr int NM = KH * NI * TM * TN, NRD = KH * NRH, SB = NM / 2 - 1;
  constexpr int UNROLL = (NS % 2 == 0) ? NS : 2 * NS;
  static_assert(G <= (NP == 2 ? 2 : 4) * (SB + 1), "not enough MFMA slots before the barrier");   // (one plane: half the units, a third of the slots)
  static_assert(A_KC || BM == 32 || BM == 64 || BM == 128, "KS image: 32, 64 or 128 columns");
  static_assert(B_KC || BN == 32 || BN == 64 || BN == 128, "KS image: 32, 64 or 128 columns");
  extern __shared__ __attribute__((aligned(1024))) float lds[];
  const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) void *)lds;
  lds_char *lds3 = (lds_char *)(__attribute__((address_space(3))) void *)lds;
  const char *ldsb = reinterpret_cast<const char *>(lds);

  const bool second = g.pair && blockIdx.z == 1;   // second product of a pair (uniform)
  if (second) { g.C = g.C1; g.ep = g.ep1; }
  const S16View va = s16_pick(second, ops.a, ops.a1), vb = s16_pick(second, ops.b, ops.b1);
  int tm, tn;
  xcd_tile<BM, BN>(g, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave / WGN, wn = wave % WGN, l31 = lane & 31, lh = lane >> 5;
  // split-K (as gemm_glds.hip): this workgroup reduces over K chunk blockIdx.y only and leaves a plain, unscaled-back partial product
  // in C + chunk * split_stride (the host has emptied the epilogue; splitk_reduce_kernel adds the chunks in order and applies it)
  int k_first = 0, ktiles = ops.kp / BKH;
  if (g.split_k > 1) {
    k_first = (int)blockIdx.y * g.k_chunk;                       // a multiple of the K tile
    ktiles = min(g.k_chunk, ops.kp - k_first) / BKH;
    g.C += (long)blockIdx.y * g.split_stride;
  }

  // ---- DMA descriptors: unit = 1 KiB of one plane tile.  KC: 8 rows x 128 B.  KS: 64 / (BR / 8) k rows x 2 BR bytes.
  const h16 *src[G];
  int adv[G];          // halves per K tile
  unsigned dst_off[G];
  static_for<0, G>([&](auto U_) {
    constexpr int u = decltype(U_)::value;
    const int slot = wave + u * NW;  // wave-uniform
    // plane order inside a stage: A_hi [0, SLOTS_A), A_lo, B_hi [2 SLOTS_A, ...), B_lo.  The plane tiles' unit counts are multiples of
    // the wave count, so WHICH plane unit u of a wave belongs to is a compile-time fact: choosing va / vb members under a run-time
    // condition makes hipcc select between their ADDRESSES, which parks both views in scratch memory (a private segment per launch)
    static_assert(SLOTS_A % NW == 0 && SLOTS_B % NW == 0, "a wave's DMA unit must not straddle planes");
    constexpr bool is_a = u * NW < NP * SLOTS_A;
    constexpr int s2c = is_a ? u * NW : u * NW - NP * SLOTS_A, per = is_a ? SLOTS_A : SLOTS_B;
    constexpr bool lo_plane = s2c >= per;
    const int sr = (lo_plane ? s2c - per : s2c) + wave;   // unit within the plane tile
    const h16 *base;
    int v_ld, v_rows;
    if constexpr (is_a) { v_ld = va.ld; v_rows = va.rows; if constexpr (lo_plane) base = va.lo; else base = va.hi; }
    else { v_ld = vb.ld; v_rows = vb.rows; if constexpr (lo_plane) base = vb.lo; else base = vb.hi; }
    const int rows_p = (v_rows + kS16Pad - 1) / kS16Pad * kS16Pad;
    auto kc_src = [&](int first_row) {
      const int r = lane >> 3;
      const int c = (lane & 7) ^ kc_swizzle(sr * 8 + r);
      int row = first_row + sr * 8 + r;
      row = row < rows_p ? row : rows_p - 1;   // (a row of the padding or of another tile: feeds outputs that are not stored)
      adv[u] = BKH;
      return base + (long)row * v_ld + 8 * c + k_first;
    };
    auto ks_src = [&](int first_col, auto BR_) {
      constexpr int BR = decltype(BR_)::value, CPR = BR / 8;   // 16-byte chunks per k row
      const int krow = sr * (64 / CPR) + lane / CPR;
      const int c = (lane % CPR) ^ (4 * ks_swizzle<BR>(krow));
      int col = first_col + 8 * c;
      col = col + 8 <= v_ld ? col : v_ld - 8;   // (columns past the planes: outputs that are not stored)
      adv[u] = BKH * v_ld;
      return base + (long)(k_first + krow) * v_ld + col;
    };
    if (is_a) {
      if constexpr (A_KC) src[u] = kc_src(m0); else src[u] = ks_src(m0, std::integral_constant<int, BM>());
    } else {
      if constexpr (B_KC) src[u] = kc_src(n0); else src[u] = ks_src(n0, std::integral_constant<int, BN>());
    }
    dst_off[u] = slot * 1024;
  });
  auto dma_unit = [&](auto U_, auto ST_, int r) {
    constexpr int u = decltype(U_)::value, st = decltype(ST_)::value;
    if constexpr (!(ABL & 2)) glds16(src[u], __builtin_amdgcn_readfirstlane(lds_base + st * STAGE + dst_off[u]));
    src[u] += (r + 1 < ktiles) ? adv[u] : 0;   // requests past the last tile fetch it again into a stage nobody reads
  };

  // ---- fragments: per-lane byte offsets inside a plane tile
  //  KC: row * 128 + swizzled 16-byte chunk (2 h + lh);  KS: lane (p = lane & 15, column half g = (lane >> 4) & 1) of a 16-lane group
  //  addresses k row 8 lh + p / 4, columns 16 g + 4 (p & 3) .. + 3 of its 32-column fragment and receives column 16 g + p, k .. k + 3
  //  (KC keeps one offset per k step: the swizzle is an XOR; KS steps are plain additions that fold into the instruction's offset field)
  constexpr int AH = A_KC ? KH : 1, BH = B_KC ? KH : 1;
  int a_off[TM][AH], b_off[TN][BH];
  const int p16 = lane & 15, g16 = (lane >> 4) & 1;
#pragma unroll
  for (int t = 0; t < TM; t++) {
    if constexpr (A_KC) {
      const int row = wm * WM + t * 32 + l31;
#pragma unroll
      for (int h = 0; h < KH; h++) a_off[t][h] = row * 128 + (((2 * h + lh) ^ kc_swizzle(row)) << 4);
    } else {
      const int T = wm * TM + t, krow = 8 * lh + (p16 >> 2);
      a_off[t][0] = krow * (2 * BM) + 64 * (T ^ ks_swizzle<BM>(krow)) + 32 * g16 + 8 * (p16 & 3);
    }
  }
#pragma unroll
  for (int t = 0; t < TN; t++) {
    if constexpr (B_KC) {
      const int col = wn * WN + t * 32 + l31;
#pragma unroll
      for (int h = 0; h < KH; h++) b_off[t][h] = NP * A_BYTES + col * 128 + (((2 * h + lh) ^ kc_swizzle(col)) << 4);
    } else {
      const int T = wn * TN + t, krow = 8 * lh + (p16 >> 2);
      b_off[t][0] = NP * A_BYTES + krow * (2 * BN) + 64 * (T ^ ks_swizzle<BN>(krow)) + 32 * g16 + 8 * (p16 & 3);
    }
  }
  struct Frag {
    half8 ah[KH][TM], al[KH][TM], bh[KH][TN], bl[KH][TN];
  };
  // one LDS read: flat index r -> (k step h, operand, fragment t, plane, half of the fragment)
  auto read_unit = [&](auto ST_, Frag &f, auto R_) {
    constexpr int r = decltype(R_)::value, st = decltype(ST_)::value;
    if constexpr (ABL & 4) return;
    constexpr int h = r / NRH, q = r % NRH;
    constexpr bool is_a = q < NP * TM * RA;
    constexpr int q2 = is_a ? q : q - NP * TM * RA, RR = is_a ? RA : RB;
    constexpr int t = q2 / (NP * RR), w = q2 % (NP * RR), lo = w / RR, half = w % RR;
    constexpr bool kc = is_a ? A_KC : B_KC;
    constexpr int plane_bytes = is_a ? A_BYTES : B_BYTES, BR = is_a ? BM : BN;
    int base = st * STAGE + (lo ? plane_bytes : 0);
    if constexpr (is_a) base += a_off[t][kc ? h : 0]; else base += b_off[t][kc ? h : 0];
    if constexpr (kc) {
      const half8 v = *reinterpret_cast<const half8 *>(ldsb + base);
      if constexpr (ABL & 1) asm volatile("" ::"v"(v));
      if constexpr (is_a) { if constexpr (lo) f.al[h][t] = v; else f.ah[h][t] = v; }
      else { if constexpr (lo) f.bl[h][t] = v; else f.bh[h][t] = v; }
    } else {
      const half4 v = __builtin_bit_cast(half4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4 *)(lds3 + base + (16 * h + 4 * half) * (2 * BR))));
      if constexpr (ABL & 1) asm volatile("" ::"v"(v));
      half8 *dst = is_a ? (lo ? &f.al[h][t] : &f.ah[h][t]) : (lo ? &f.bl[h][t] : &f.bh[h][t]);
      if constexpr (half == 0) dst->lo = v; else dst->hi = v;
    }
  };

  // (NP == 1: accx and the lo members of Frag are never touched by a matrix instruction or a read and cost no register -- kept so that
  // the one template serves both plane counts)
  f32x16 acc[TM][TN], accx[TM][TN];   // hi hi; hi lo' + lo' hi
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int j = 0; j < TN; j++)
#pragma unroll
      for (int e = 0; e < 16; e++) { acc[i][j][e] = 0.0f; accx[i][j][e] = 0.0f; }
  // optional column sums of a reduction-major A operand (the bias gradient on the weight-gradient product, as gemm_glds.hip): the
  // first column of tiles' wn == 0 waves add up the A pieces they multiply anyway -- sum_k (hi + 2^-11 lo'), unscaled at the end
  const bool do_colsum = !A_KC && g.ep.colsum != nullptr && tn == 0 && wn == 0;  // wave-uniform
  float asum[TM];
#pragma unroll
  for (int i = 0; i < TM; i++) asum[i] = 0.0f;
  auto colsum_unit = [&](const Frag &f) {
    typedef _Float16 half2v __attribute__((ext_vector_type(2)));
    const half2v one = {(h16)1.0f, (h16)1.0f}, eps = {(h16)0x1p-11f, (h16)0x1p-11f};
#pragma unroll
    for (int h = 0; h < KH; h++)
#pragma unroll
      for (int i = 0; i < TM; i++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const half2v hv = {f.ah[h][i][2 * q], f.ah[h][i][2 * q + 1]};
          asum[i] = __builtin_amdgcn_fdot2(hv, one, asum[i], false);     // fp32 accumulation of exact fp16 values
          if constexpr (NP == 2) {   // (one plane: the lo fragments are never read -- the sums are those of the operand the product multiplies)
            const half2v lv = {f.al[h][i][2 * q], f.al[h][i][2 * q + 1]};
            asum[i] = __builtin_amdgcn_fdot2(lv, eps, asum[i], false);
          }
        }
  };
  auto mma_unit = [&](const Frag &f, auto M_) {
    constexpr int m = decltype(M_)::value;
    if constexpr (ABL & 1) return;
    constexpr int n = m % TN, i = (m / TN) % TM, j = (m / (TN * TM)) % NI, h = m / (TN * TM * NI);
    if constexpr (j == 0) acc[i][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ah[h][i], f.bh[h][n], acc[i][n], 0, 0, 0);
    else if constexpr (j == 1) accx[i][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ah[h][i], f.bl[h][n], accx[i][n], 0, 0, 0);
    else accx[i][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.al[h][i], f.bh[h][n], accx[i][n], 0, 0, 0);
  };

  auto step = [&](auto I_, const Frag &fcur, Frag &fnxt, int t) {
    constexpr int I = decltype(I_)::value;
    using StReq = std::integral_constant<int, (I + D) % NS>;
    using StNxt = std::integral_constant<int, (I + 1) % NS>;
    static_for<0, NM>([&](auto S_) {
      constexpr int sidx = decltype(S_)::value;
      mma_unit(fcur, S_);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (!A_KC && sidx == 0) {
        if (do_colsum) colsum_unit(fcur);
      }
      if constexpr (sidx <= SB) {
        static_for<sidx * G / (SB + 1), (sidx + 1) * G / (SB + 1)>([&](auto U_) { dma_unit(U_, StReq(), t + D); });
        if constexpr (sidx == SB) {
          wait_vmcnt<(D - 1) * G>();
          __builtin_amdgcn_s_barrier();
          asm volatile("" ::: "memory");
        }
      } else {
        constexpr int NSL = NM - SB - 1;
        static_for<(sidx - SB - 1) * NRD / NSL, (sidx - SB) * NRD / NSL>([&](auto R_) { read_unit(StNxt(), fnxt, R_); });
      }
      __builtin_amdgcn_sched_barrier(0);
    });
  };

  Frag f0, f1;
  if constexpr (ABL & 4) {   // fragments never read: give them defined (non-constant) contents
    half8 z;
#pragma unroll
    for (int e = 0; e < 8; e++) z[e] = (h16)(float)(lane + e);
    static_for<0, KH>([&](auto H_) {
      constexpr int h = decltype(H_)::value;
#pragma unroll
      for (int t = 0; t < TM; t++) { f0.ah[h][t] = z; f0.al[h][t] = z; f1.ah[h][t] = z; f1.al[h][t] = z; }
#pragma unroll
      for (int t = 0; t < TN; t++) { f0.bh[h][t] = z; f0.bl[h][t] = z; f1.bh[h][t] = z; f1.bl[h][t] = z; }
    });
  }
  static_for<0, D>([&](auto T_) {
    constexpr int t = decltype(T_)::value;
    static_for<0, G>([&](auto U_) { dma_unit(U_, T_, t); });
  });
  float w_bound = 0.f;
  if constexpr (EXTRA) w_bound = s16_weight_bound(g, va, vb, lane);   // while the first tiles are on their way
  wait_vmcnt<(D - 1) * G>();
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  static_for<0, NRD>([&](auto R_) { read_unit(std::integral_constant<int, 0>(), f0, R_); });

  for (int t0 = 0; t0 < ktiles; t0 += UNROLL) {
    static_for<0, UNROLL>([&](auto I_) {
      constexpr int I = decltype(I_)::value;
      if (t0 + I < ktiles) {  // wave-uniform
        if constexpr (I % 2 == 0) step(I_, f0, f1, t0 + I);
        else step(I_, f1, f0, t0 + I);
      }
    });
  }
  wait_vmcnt<0>();

  static_assert(NW * 32 * kEpiPitch * (int)sizeof(float) <= NS * STAGE, "the waves' epilogue slices must fit into the operand LDS");
  s16_finish<TM, TN, NW, EXTRA, !A_KC, NP>(g, va, vb, acc, accx, asum, do_colsum, w_bound, m0 + wm * WM, n0 + wn * WN, lane, wave, lds);
}

// ---- both operands reduction-major (the weight gradient dW = dy^T x), 128 x 128 tile ---------------------------------------------
// The generic kernel above keeps the fragments of a whole 64-deep K tile in registers, twice: with a 128 x 128 tile on four waves that is
// 256 registers of fragments beside 128 of accumulators, and the transposing reads' addresses push it into scratch memory.  Here the
// tile's depth is 32 (two instruction steps), the fragments are double buffered per instruction step (64 registers), and the LDS holds a
// ring of FOUR such half tiles (128 KB): the DMA runs three half tiles (~2300 matrix-pipe cycles) ahead of the reads.  Against the
// 64 x 128 tile the 128 x 128 one moves a third less through L2 -> LDS per flop and issues a third fewer LDS reads per MFMA (wave tile
// 64 x 64) -- the two things gemm_s16_glds waits for (devtools/micro/s16_ablate.hip).
//   half tile h, slot h % 4:  A_hi | A_lo | B_hi | B_lo, each [32 k][128 columns] halves = 8 KB, rows as they lie in memory
//   per half tile and wave: 8 DMA units (4 k rows x 256 B each), 2 x 12 MFMAs, 2 x 16 transposing reads, one barrier
template <bool EXTRA>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) gemm_s16_ks128(GemmArgs g, S16Operands ops) {   // (128 KB of LDS: one workgroup per CU whatever the register count)
  constexpr int BM = 128, BN = 128, NW = 4, TM = 2, TN = 2, KT = 32, RING = 4;
  constexpr int PLANE = KT * BM * 2, SLOT = 4 * PLANE;      // bytes: 8 KB per plane, 32 KB per half tile
  constexpr int G = (4 * PLANE / 1024) / NW;                  // 8 DMA units per wave and half tile
  extern __shared__ __attribute__((aligned(1024))) float lds[];
  const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) void *)lds;
  lds_char *lds3 = (lds_char *)(__attribute__((address_space(3))) void *)lds;

  const bool second = g.pair && blockIdx.z == 1;   // second product of a pair (uniform)
  if (second) { g.C = g.C1; g.ep = g.ep1; }
  const S16View va = s16_pick(second, ops.a, ops.a1), vb = s16_pick(second, ops.b, ops.b1);
  int tm, tn;
  xcd_tile<BM, BN>(g, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1, lh = lane >> 5;
  const int htiles = ops.kp / KT;

  // ---- DMA descriptors: unit = 4 k rows x 256 B of one plane; plane p = unit / 8 (A_hi, A_lo, B_hi, B_lo), 8 units per plane
  const h16 *src[G];
  int adv[G];
  static_for<0, G>([&](auto U_) {
    constexpr int u = decltype(U_)::value;
    // (8 units per plane, 4 waves: the plane of a wave's unit u is a compile-time fact -- see gemm_s16_glds)
    constexpr int plane = (u * NW) >> 3;
    const int sub = (wave + u * NW) & 7;
    constexpr bool is_a = plane < 2, lo_plane = (plane & 1) != 0;
    const h16 *base;
    int v_ld;
    if constexpr (is_a) { v_ld = va.ld; if constexpr (lo_plane) base = va.lo; else base = va.hi; }
    else { v_ld = vb.ld; if constexpr (lo_plane) base = vb.lo; else base = vb.hi; }
    const int krow = sub * 4 + (lane >> 4);
    const int c = (lane & 15) ^ (4 * (krow & 3));   // the 64-byte column groups of a k row, XOR-swizzled with the row's low bits
    int col = (is_a ? m0 : n0) + 8 * c;
    col = col + 8 <= v_ld ? col : v_ld - 8;         // (columns past the planes: outputs that are not stored)
    src[u] = base + (long)krow * v_ld + col;
    adv[u] = KT * v_ld;
  });
  auto dma_half_tile = [&](int slot, int h) {   // slot: wave-uniform ring index
    static_for<0, G>([&](auto U_) {
      constexpr int u = decltype(U_)::value;
      glds16(src[u], __builtin_amdgcn_readfirstlane(lds_base + slot * SLOT + (wave + u * NW) * 1024));
      src[u] += (h + 1 < htiles) ? adv[u] : 0;   // requests past the last half tile fetch it again into a slot nobody reads
    });
  };
  auto dma_unit = [&](auto U_, int slot, int h) {
    constexpr int u = decltype(U_)::value;
    glds16(src[u], __builtin_amdgcn_readfirstlane(lds_base + slot * SLOT + (wave + u * NW) * 1024));
    src[u] += (h + 1 < htiles) ? adv[u] : 0;
  };

  // ---- fragment addresses (bytes inside a slot): lane (p = lane & 15, column half gg) addresses k row 8 lh + p / 4 of its 16-lane group's
  // [4 k][16 columns] block and receives column 16 gg + p, k .. k + 3 (ds_read_b64_tr_b16)
  const int p16 = lane & 15, gg = (lane >> 4) & 1, krow_l = 8 * lh + (p16 >> 2);
  int a_off[TM], b_off[TN];
#pragma unroll
  for (int t = 0; t < TM; t++) a_off[t] = krow_l * 256 + 64 * ((wm * TM + t) ^ (krow_l & 3)) + 32 * gg + 8 * (p16 & 3);
#pragma unroll
  for (int t = 0; t < TN; t++) b_off[t] = 2 * PLANE + krow_l * 256 + 64 * ((wn * TN + t) ^ (krow_l & 3)) + 32 * gg + 8 * (p16 & 3);
  struct Frag { half8 ah[TM], al[TM], bh[TN], bl[TN]; };   // one instruction step
  // read r of the 16 of an instruction step: operand, fragment, plane, half of the fragment
  auto read_unit = [&](int slot_base, auto KS_, Frag &f, auto R_) {
    constexpr int r = decltype(R_)::value, ks = decltype(KS_)::value;
    constexpr bool is_a = r < 8;
    constexpr int q = r & 7, t = q >> 2, lo = (q >> 1) & 1, half = q & 1;
    const int off = slot_base + (is_a ? a_off[t] : b_off[t]) + (lo ? PLANE : 0) + (16 * ks + 4 * half) * 256;
    const half4 v = __builtin_bit_cast(half4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4 *)(lds3 + off)));
    half8 *dst = is_a ? (lo ? &f.al[t] : &f.ah[t]) : (lo ? &f.bl[t] : &f.bh[t]);
    if constexpr (half == 0) dst->lo = v; else dst->hi = v;
  };

  f32x16 acc[TM][TN], accx[TM][TN];   // hi hi; hi lo' + lo' hi
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int j = 0; j < TN; j++)
#pragma unroll
      for (int e = 0; e < 16; e++) { acc[i][j][e] = 0.0f; accx[i][j][e] = 0.0f; }
  const bool do_colsum = g.ep.colsum != nullptr && tn == 0 && wn == 0;  // wave-uniform
  float asum[TM] = {0.f, 0.f};
  // MFMA m of the 12 of an instruction step: the four main products, then the four hi lo', then the four lo' hi (a cross accumulator is
  // met again four instructions later)
  auto mma_unit = [&](const Frag &f, auto M_) {
    constexpr int m = decltype(M_)::value, j = m >> 2, i = (m >> 1) & 1, n = m & 1;
    if constexpr (j == 0) acc[i][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ah[i], f.bh[n], acc[i][n], 0, 0, 0);
    else if constexpr (j == 1) accx[i][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ah[i], f.bl[n], accx[i][n], 0, 0, 0);
    else accx[i][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.al[i], f.bh[n], accx[i][n], 0, 0, 0);
  };

  // prologue: three half tiles on their way, the first one landed, its first step's fragments read
  Frag f0, f1;
  dma_half_tile(0, 0);
  dma_half_tile(1, 1);
  dma_half_tile(2, 2);
  float w_bound = 0.f;
  if constexpr (EXTRA) w_bound = s16_weight_bound(g, va, vb, lane);
  wait_vmcnt<2 * G>();
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  static_for<0, 16>([&](auto R_) { read_unit(0, std::integral_constant<int, 0>(), f0, R_); });

  for (int h = 0; h < htiles; h++) {
    const int slot = h & (RING - 1), slot_base = slot * SLOT;
    const int slot_req = (h + 3) & (RING - 1), slot_nxt = ((h + 1) & (RING - 1)) * SLOT;
    // step 0 of half tile h from f0: request half tile h + 3 (the slot of h - 1: every wave has passed the barrier behind its last
    // read of it), read step 1's fragments into f1
    static_for<0, 12>([&](auto S_) {
      constexpr int sidx = decltype(S_)::value;
      mma_unit(f0, S_);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (sidx == 0) {
        if (do_colsum) {
#pragma unroll
          for (int i = 0; i < TM; i++) asum[i] = s16_frag_sum(asum[i], f0.ah[i], f0.al[i]);
        }
      }
      if constexpr (sidx < G) dma_unit(S_, slot_req, h + 3);
      static_for<sidx * 16 / 12, (sidx + 1) * 16 / 12>([&](auto R_) { read_unit(slot_base, std::integral_constant<int, 1>(), f1, R_); });
      __builtin_amdgcn_sched_barrier(0);
    });
    // step 1 from f1: this wave's share of half tile h + 1 has landed (h + 2, h + 3 stay in flight), one barrier publishes it, then
    // its first step's fragments go into f0
    static_for<0, 12>([&](auto S_) {
      constexpr int sidx = decltype(S_)::value;
      mma_unit(f1, S_);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (sidx == 0) {
        if (do_colsum) {
#pragma unroll
          for (int i = 0; i < TM; i++) asum[i] = s16_frag_sum(asum[i], f1.ah[i], f1.al[i]);
        }
      }
      if constexpr (sidx == 3) {
        wait_vmcnt<2 * G>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
      }
      if constexpr (sidx >= 4) {
        static_for<(sidx - 4) * 16 / 8, (sidx - 3) * 16 / 8>([&](auto R_) { read_unit(slot_nxt, std::integral_constant<int, 0>(), f0, R_); });
      }
      __builtin_amdgcn_sched_barrier(0);
    });
  }
  wait_vmcnt<0>();
  static_assert(NW * 32 * kEpiPitch * (int)sizeof(float) <= RING * SLOT, "the waves' epilogue slices must fit into the operand LDS");
  s16_finish<TM, TN, NW, EXTRA, true>(g, va, vb, acc, accx, asum, do_colsum, w_bound, m0 + wm * 64, n0 + wn * 64, lane, wave, lds);
}

// ---- producer / consumer waves (round 6) -------------------------------------------------------------------------------------------
// The kernels above run one wave per SIMD that does everything: it issues the K tile's LDS-DMA requests, the fragment reads and the
// matrix instructions from ONE in-order instruction stream.  The counters (profiles/r06_gemm_split16_pmc_*.txt) say what that costs:
// 40 % of the wave cycles are instruction-issue stalls (SQ_WAIT_INST_ANY) while the LDS is ~25 % busy with no bank conflicts and the
// matrix pipe ~45 % busy -- a global_load_lds that waits for the texture path to take it (one 1-KiB request per ~70 cycles and wave at the
// path's ~56 B/clk/CU) holds up the matrix instructions and reads behind it, and nothing else can issue on that SIMD.  Here a workgroup
// is EIGHT waves, two per SIMD: waves 0-3 (consumers) only read fragments and multiply, waves 4-7 (producers) only issue the LDS-DMA
// requests and wait for them; a producer parked on the texture path costs its SIMD nothing, the consumer beside it keeps issuing.  One
// workgroup barrier per K tile connects the two roles exactly as before (counted vmcnt on the producer side, then the barrier publishes
// the tile and frees the stage the consumers have just left).  Producers end behind the K loop; the epilogue's barriers then count the
// surviving consumer waves only.  Same instruction order per accumulator as the kernels above: results are bit-identical to theirs.
//   KT = 64 halves per K tile (KC operands need 128-byte rows for their LDS image) or 32 when both operands are reduction-major
//   fragments double-buffered per INSTRUCTION step (registers: at most 256 per wave with two waves per SIMD)
// ABL (devtools only): 1 = no MFMA, 2 = no DMA, 4 = no LDS reads -- wrong results, for timing
template <int BM, int BN, int KT, int NS, bool A_KC, bool B_KC, bool EXTRA, int ABL = 0>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) gemm_s16_pc(GemmArgs g, S16Operands ops) {
  constexpr int NC = 4, NP = 4;   // consumer waves (2 x 2 wave tiles), producer waves
  constexpr int WM = BM / 2, WN = BN / 2, TM = WM / 32, TN = WN / 32;
  constexpr int KHS = KT / 16;    // instruction k steps per K tile
  static_assert(KT == 64 || (KT == 32 && !A_KC && !B_KC), "an operand whose reduction index is contiguous needs 128-byte rows in its LDS image");
  static_assert(KHS % 2 == 0, "the two fragment sets alternate per step and every tile starts on the first");
  constexpr int A_BYTES = BM * KT * 2, B_BYTES = BN * KT * 2, STAGE = 2 * (A_BYTES + B_BYTES);   // A_hi | A_lo | B_hi | B_lo
  constexpr int SLOTS_A = A_BYTES / 1024, SLOTS_B = B_BYTES / 1024, SLOTS = 2 * (SLOTS_A + SLOTS_B);   // 1-KiB DMA units per plane tile
  static_assert(SLOTS_A % NP == 0 && SLOTS_B % NP == 0, "a producer's DMA unit must not straddle planes");
  constexpr int G = SLOTS / NP;
  constexpr int RA = A_KC ? 1 : 2, RB = B_KC ? 1 : 2;   // LDS reads per fragment and plane
  constexpr int NRH = 2 * (TM * RA + TN * RB);            // reads per instruction step
  constexpr int NMS = 3 * TM * TN;                        // matrix instructions per instruction step
  constexpr int BAR_AT = NMS >= 12 ? 3 : 0;               // behind which instruction of a tile's last step the barrier sits
  static_assert(A_KC || BM == 64 || BM == 128, "KS image: 64 or 128 columns");
  static_assert(B_KC || BN == 64 || BN == 128, "KS image: 64 or 128 columns");
  extern __shared__ __attribute__((aligned(1024))) float lds[];
  const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) void *)lds;
  lds_char *lds3 = (lds_char *)(__attribute__((address_space(3))) void *)lds;
  const char *ldsb = reinterpret_cast<const char *>(lds);

  const bool second = g.pair && blockIdx.z == 1;   // second product of a pair (uniform)
  if (second) { g.C = g.C1; g.ep = g.ep1; }
  const S16View va = s16_pick(second, ops.a, ops.a1), vb = s16_pick(second, ops.b, ops.b1);
  int tm, tn;
  xcd_tile<BM, BN>(g, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int k_first = 0, ktiles = ops.kp / KT;
  if (g.split_k > 1) {   // (as gemm_s16_glds: this workgroup reduces over K chunk blockIdx.y and leaves a plain partial product)
    k_first = (int)blockIdx.y * g.k_chunk;
    ktiles = min(g.k_chunk, ops.kp - k_first) / KT;
    g.C += (long)blockIdx.y * g.split_stride;
  }

  if (wave >= NC) {
    // ================================================= producer =================================================
    const int pw = wave - NC;
    const h16 *src[G];
    int adv[G];
    static_for<0, G>([&](auto U_) {
      constexpr int u = decltype(U_)::value;
      constexpr bool is_a = u * NP < 2 * SLOTS_A;
      constexpr int s2c = is_a ? u * NP : u * NP - 2 * SLOTS_A, per = is_a ? SLOTS_A : SLOTS_B;
      constexpr bool lo_plane = s2c >= per;
      const int sr = (lo_plane ? s2c - per : s2c) + pw;   // unit within the plane tile
      const h16 *base;
      int v_ld, v_rows;
      if constexpr (is_a) { v_ld = va.ld; v_rows = va.rows; if constexpr (lo_plane) base = va.lo; else base = va.hi; }
      else { v_ld = vb.ld; v_rows = vb.rows; if constexpr (lo_plane) base = vb.lo; else base = vb.hi; }
      constexpr bool kc = is_a ? A_KC : B_KC;
      constexpr int BR = is_a ? BM : BN;
      const int first = is_a ? m0 : n0;
      if constexpr (kc) {   // 8 rows x 128 B per unit, 16-byte chunks XOR-swizzled on the source side
        const int rows_p = (v_rows + kS16Pad - 1) / kS16Pad * kS16Pad;
        const int r = lane >> 3, c = (lane & 7) ^ kc_swizzle(sr * 8 + r);
        int row = first + sr * 8 + r;
        row = row < rows_p ? row : rows_p - 1;   // (a row of the padding or of another tile: feeds outputs that are not stored)
        adv[u] = KT;
        src[u] = base + (long)row * v_ld + 8 * c + k_first;
      } else {              // 1024 / (2 BR) k rows x 2 BR bytes per unit
        constexpr int CPR = BR / 8;
        const int krow = sr * (64 / CPR) + lane / CPR;
        const int c = (lane % CPR) ^ (4 * ks_swizzle<BR>(krow));
        int col = first + 8 * c;
        col = col + 8 <= v_ld ? col : v_ld - 8;   // (columns past the planes: outputs that are not stored)
        adv[u] = KT * v_ld;
        src[u] = base + (long)(k_first + krow) * v_ld + col;
      }
    });
    auto dma_tile = [&](auto ST_, int r) {   // K tile r into stage ST
      constexpr int st = decltype(ST_)::value;
      static_for<0, G>([&](auto U_) {
        constexpr int u = decltype(U_)::value;
        if constexpr (!(ABL & 2)) glds16(src[u], __builtin_amdgcn_readfirstlane(lds_base + st * STAGE + (pw + u * NP) * 1024));
        src[u] += (r + 1 < ktiles) ? adv[u] : 0;   // requests past the last tile fetch it again into a stage nobody reads any more
      });
    };
    static_for<0, NS - 1>([&](auto T_) { dma_tile(T_, decltype(T_)::value); });
    wait_vmcnt<G *(NS - 2)>();   // tile 0 has landed
    __builtin_amdgcn_s_barrier();
    for (int t0 = 0; t0 < ktiles; t0 += NS) {
      static_for<0, NS>([&](auto I_) {
        constexpr int I = decltype(I_)::value;
        if (t0 + I < ktiles) {   // uniform
          // the stage of tile t - 1: every consumer passed the barrier of tile t - 1 behind its last read of it
          dma_tile(std::integral_constant<int, (I + NS - 1) % NS>(), t0 + I + NS - 1);
          wait_vmcnt<G *(NS - 2)>();   // this wave's share of tile t + 1 has landed
          __builtin_amdgcn_s_barrier();
        }
      });
    }
    wait_vmcnt<0>();                 // (the surplus requests write into the LDS the epilogue is about to use)
    __builtin_amdgcn_s_barrier();
    return;
  }

  // =================================================== consumer ===================================================
  const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, lh = lane >> 5;
  constexpr int AH = A_KC ? KHS : 1, BH = B_KC ? KHS : 1;
  int a_off[TM][AH], b_off[TN][BH];
  const int p16 = lane & 15, g16 = (lane >> 4) & 1;
#pragma unroll
  for (int t = 0; t < TM; t++) {
    if constexpr (A_KC) {
      const int row = wm * WM + t * 32 + l31;
#pragma unroll
      for (int h = 0; h < KHS; h++) a_off[t][h] = row * 128 + (((2 * h + lh) ^ kc_swizzle(row)) << 4);
    } else {
      const int T = wm * TM + t, krow = 8 * lh + (p16 >> 2);
      a_off[t][0] = krow * (2 * BM) + 64 * (T ^ ks_swizzle<BM>(krow)) + 32 * g16 + 8 * (p16 & 3);
    }
  }
#pragma unroll
  for (int t = 0; t < TN; t++) {
    if constexpr (B_KC) {
      const int col = wn * WN + t * 32 + l31;
#pragma unroll
      for (int h = 0; h < KHS; h++) b_off[t][h] = 2 * A_BYTES + col * 128 + (((2 * h + lh) ^ kc_swizzle(col)) << 4);
    } else {
      const int T = wn * TN + t, krow = 8 * lh + (p16 >> 2);
      b_off[t][0] = 2 * A_BYTES + krow * (2 * BN) + 64 * (T ^ ks_swizzle<BN>(krow)) + 32 * g16 + 8 * (p16 & 3);
    }
  }
  struct Frag { half8 ah[TM], al[TM], bh[TN], bl[TN]; };   // one instruction step
  // LDS read r of instruction step h of the tile in stage st: operand, fragment t, plane, half of the fragment
  auto read_unit = [&](auto ST_, auto H_, Frag &f, auto R_) {
    constexpr int r = decltype(R_)::value, st = decltype(ST_)::value, h = decltype(H_)::value;
    if constexpr (ABL & 4) return;
    constexpr bool is_a = r < 2 * TM * RA;
    constexpr int q2 = is_a ? r : r - 2 * TM * RA, RR = is_a ? RA : RB;
    constexpr int t = q2 / (2 * RR), w = q2 % (2 * RR), lo = w / RR, half = w % RR;
    constexpr bool kc = is_a ? A_KC : B_KC;
    constexpr int plane_bytes = is_a ? A_BYTES : B_BYTES, BR = is_a ? BM : BN;
    int base = st * STAGE + (lo ? plane_bytes : 0);
    if constexpr (is_a) base += a_off[t][kc ? h : 0]; else base += b_off[t][kc ? h : 0];
    if constexpr (kc) {
      const half8 v = *reinterpret_cast<const half8 *>(ldsb + base);
      if constexpr (is_a) { if constexpr (lo) f.al[t] = v; else f.ah[t] = v; }
      else { if constexpr (lo) f.bl[t] = v; else f.bh[t] = v; }
    } else {
      const half4 v = __builtin_bit_cast(half4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4 *)(lds3 + base + (16 * h + 4 * half) * (2 * BR))));
      half8 *dst = is_a ? (lo ? &f.al[t] : &f.ah[t]) : (lo ? &f.bl[t] : &f.bh[t]);
      if constexpr (half == 0) dst->lo = v; else dst->hi = v;
    }
  };

  f32x16 acc[TM][TN], accx[TM][TN];   // hi hi; hi lo' + lo' hi
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int j = 0; j < TN; j++)
#pragma unroll
      for (int e = 0; e < 16; e++) { acc[i][j][e] = 0.0f; accx[i][j][e] = 0.0f; }
  const bool do_colsum = !A_KC && g.ep.colsum != nullptr && tn == 0 && wn == 0;  // wave-uniform
  float asum[TM];
#pragma unroll
  for (int i = 0; i < TM; i++) asum[i] = 0.0f;
  // matrix instruction m of a step: all main products, then all hi lo', then all lo' hi (an accumulator is met again TM TN instructions later)
  auto mma_unit = [&](const Frag &f, auto M_) {
    constexpr int m = decltype(M_)::value;
    constexpr int n = m % TN, i = (m / TN) % TM, j = m / (TN * TM);
    if constexpr (ABL & 1) {   // the instruction's operands are waited for where it would issue, nothing more
      if constexpr (j == 0) asm volatile("" ::"v"(f.ah[i]), "v"(f.bh[n]));
      else if constexpr (j == 1) asm volatile("" ::"v"(f.bl[n]));
      else asm volatile("" ::"v"(f.al[i]));
      return;
    }
    if constexpr (j == 0) acc[i][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ah[i], f.bh[n], acc[i][n], 0, 0, 0);
    else if constexpr (j == 1) accx[i][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ah[i], f.bl[n], accx[i][n], 0, 0, 0);
    else accx[i][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.al[i], f.bh[n], accx[i][n], 0, 0, 0);
  };
  // instruction step h of the tile in stage st from fc; the next step's fragments go into fn -- behind the tile's barrier when they
  // belong to the next tile
  auto cstep = [&](auto ST_, auto H_, const Frag &fc, Frag &fn) {
    constexpr int st = decltype(ST_)::value, h = decltype(H_)::value;
    constexpr bool last = h == KHS - 1;
    using StN = std::integral_constant<int, last ? (st + 1) % NS : st>;
    using HN = std::integral_constant<int, last ? 0 : h + 1>;
    constexpr int first = last ? BAR_AT : 0, nslots = NMS - first;
    static_for<0, NMS>([&](auto S_) {
      constexpr int s = decltype(S_)::value;
      mma_unit(fc, S_);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (!A_KC && s == 0) {
        if (do_colsum) {
#pragma unroll
          for (int i = 0; i < TM; i++) asum[i] = s16_frag_sum(asum[i], fc.ah[i], fc.al[i]);
        }
      }
      if constexpr (last && s == BAR_AT) {
        __builtin_amdgcn_s_barrier();   // the next tile has landed; the producers may refill this one's stage
        asm volatile("" ::: "memory");
      }
      if constexpr (s >= first) {
        static_for<(s - first) * NRH / nslots, (s - first + 1) * NRH / nslots>([&](auto R_) { read_unit(StN(), HN(), fn, R_); });
      }
      __builtin_amdgcn_sched_barrier(0);
    });
  };

  Frag f0, f1;
  if constexpr (ABL & 4) {   // fragments never read: give them defined (non-constant) contents
    half8 z;
#pragma unroll
    for (int e = 0; e < 8; e++) z[e] = (h16)(float)(lane + e);
#pragma unroll
    for (int t = 0; t < TM; t++) { f0.ah[t] = z; f0.al[t] = z; f1.ah[t] = z; f1.al[t] = z; }
#pragma unroll
    for (int t = 0; t < TN; t++) { f0.bh[t] = z; f0.bl[t] = z; f1.bh[t] = z; f1.bl[t] = z; }
  }
  float w_bound = 0.f;
  if constexpr (EXTRA) w_bound = s16_weight_bound(g, va, vb, lane);   // while the first tiles are on their way
  __builtin_amdgcn_s_barrier();   // tile 0 has landed
  asm volatile("" ::: "memory");
  static_for<0, NRH>([&](auto R_) { read_unit(std::integral_constant<int, 0>(), std::integral_constant<int, 0>(), f0, R_); });
  for (int t0 = 0; t0 < ktiles; t0 += NS) {
    static_for<0, NS>([&](auto I_) {
      constexpr int I = decltype(I_)::value;
      if (t0 + I < ktiles) {  // wave-uniform
        static_for<0, KHS>([&](auto H_) {
          if constexpr (decltype(H_)::value % 2 == 0) cstep(I_, H_, f0, f1);
          else cstep(I_, H_, f1, f0);
        });
      }
    });
  }
  __builtin_amdgcn_s_barrier();   // the producers' last requests have landed: the operand LDS is the epilogue's now
  asm volatile("" ::: "memory");
  static_assert(NC * 32 * kEpiPitch * (int)sizeof(float) <= NS * STAGE, "the waves' epilogue slices must fit into the operand LDS");
  s16_finish<TM, TN, NC, EXTRA, !A_KC>(g, va, vb, acc, accx, asum, do_colsum, w_bound, m0 + wm * WM, n0 + wn * WN, lane, wave, lds);
}

}  // namespace
}  // namespace aslp
