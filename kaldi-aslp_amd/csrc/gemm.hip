// gemm.hip -- fp32 GEMM on the CDNA4 matrix cores (v_mfma_f32_32x32x2_f32) for gfx950.
//
// Replaces the cuBLAS sgemm seam (src/aslp-cudamatrix/cublas-wrappers.h:28-47, call site
// CuMatrixBase::AddMatMat cu-matrix.cc:1027-1061): row-major
//     C[M x N] = alpha * op(A) * op(B) + beta * C   (+ fused epilogue, see aslp_kernels.h)
// gfx950 has no xf32/TF32 path: the f32-input MFMA is exact fp32 (bitwise an fmaf chain) at
// 157.3 TFLOP/s peak, which is what keeps Propagate/Backpropagate inside the 1e-4 parity bar.
//
// Tiling (4 or 8 waves, one or two per SIMD; each wave owns a (BM/WGM) x (BN/WGN) patch
// made of 32x32 MFMA tiles; accumulators stay in registers for the whole K loop):
//   * operands whose K index is contiguous in memory ("KC": A of NT/NN, B of NT) are staged
//     as [rows][BK+4] and read back with ONE ds_read_b128 per 4 MFMA k-steps: lane l takes
//     k = 8*h + 4*(l>>5) + {0..3} of row (l&31).  The +4 pad makes the 16-lane b128 groups
//     conflict-free (stride 20 dwords = 5 slots, odd).
//   * operands whose row index is contiguous ("RC": A of TN, B of NN/TN) are staged as
//     [BK][rows+4] and read with ds_read_b32 using the SAME k permutation, so both operands
//     of one MFMA agree on which two k's a step consumes.
//   * global->LDS goes through registers (float4 per lane, coalesced along the contiguous
//     dimension), double-buffered in LDS: the loads of tile t+1 are issued before the MFMAs
//     of tile t and written to the other buffer after them -- one barrier per K tile.
// The K order inside a tile is a permutation of 0..BK-1; fp32 sums are therefore not
// bitwise those of a k-ascending loop (parity is tolerance-based for GEMM rows).
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

#include "gemm_common.h"
#include "split16.h"

namespace aslp {
namespace {

// One staged operand tile of BR rows x BK reduction steps, moved by NT threads.  KC: [BR][BK + 4] in LDS, RC: [BK][BR + 4].  Thread t
// moves the float4 numbered idx = t + i * NT, i < NV: the 4 floats from 4 * (idx % C4) of run idx / C4, where a run is a row of a KC
// tile and a k of an RC tile -- the one index mapping of the global load, the LDS store and the LDS layout.
template <int BR, int BK, int NT, bool KC>
struct Stage {
  static constexpr int TOTAL = BR * BK / 4;          // float4 per tile
  static constexpr int NV = (TOTAL + NT - 1) / NT;   // float4 per thread per tile
  static constexpr bool FULL = TOTAL % NT == 0;      // otherwise the tail threads idle
  static constexpr int C4 = (KC ? BK : BR) / 4;      // float4 per run
  static constexpr int LD = (KC ? BK : BR) + 4;      // LDS stride of a run (KC: an odd number of 16-byte slots)
  static constexpr int kFloats = (KC ? BR : BK) * LD;
};

// ---- global -> registers ------------------------------------------------------------------
// src is [R x K] row-major (KC) or [K x R] row-major (RC) with leading dimension ld; the tile starts at row r0, reduction step k0.
// The VEC form is branch-free: addresses are clamped into the matrix and out-of-range k is zeroed with a select at LDS-store time, so
// the loads of one tile issue back to back with no s_waitcnt between them (hipcc serialises "branch around each load" forms, cdna
// guide §5 trap (c)).  It needs 16-byte aligned pointers / strides and the contiguous extent to be a multiple of 4.
// Rows beyond the matrix are clamped (they only feed accumulator rows that are never stored).
template <int BR, int BK, int NT, bool KC, bool VEC>
__device__ __forceinline__ void gload(const float *__restrict__ src, int ld, int R, int K, int r0, int k0,
                                      float4 (&v)[Stage<BR, BK, NT, KC>::NV]) {
  typedef Stage<BR, BK, NT, KC> S;
#pragma unroll
  for (int i = 0; i < S::NV; i++) {
    const int idx = threadIdx.x + i * NT;
    const int run = idx / S::C4, c = idx % S::C4 * 4;
    int gr = r0 + (KC ? run : c);
    const int gk = k0 + (KC ? c : run);
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (VEC) {
      if (S::FULL || idx < S::TOTAL) {
        const bool kv = gk < K;  // (KC: K % 4 == 0, the whole float4 is in or out)   masked at store time
        if constexpr (KC) {
          gr = gr < R ? gr : R - 1;
          x = *reinterpret_cast<const float4 *>(src + (long)gr * ld + (kv ? gk : 0));
        } else {
          gr = gr + 3 < R ? gr : R - 4;  // R % 4 == 0
          x = *reinterpret_cast<const float4 *>(src + (long)(kv ? gk : 0) * ld + gr);
        }
      }
    } else {  // element by element: run `o` of the matrix, elements e .. e + 3 along it
      const int o = KC ? gr : gk, o_end = KC ? R : K, e = KC ? gk : gr, e_end = KC ? K : R;
      if ((S::FULL || idx < S::TOTAL) && o < o_end) {
        const float *p = src + (long)o * ld + e;
        if (e < e_end) x.x = p[0];
        if (e + 1 < e_end) x.y = p[1];
        if (e + 2 < e_end) x.z = p[2];
        if (e + 3 < e_end) x.w = p[3];
      }
    }
    v[i] = x;
  }
}
// registers -> LDS.  The k-tail zeroing of the VEC loads happens here: touching the loaded registers right after the load would
// make the compiler wait for them (vmcnt) immediately and kill the prefetch distance.
template <int BR, int BK, int NT, bool KC, bool VEC>
__device__ __forceinline__ void sstore(float *lds, const float4 (&v)[Stage<BR, BK, NT, KC>::NV], int k0, int K) {
  typedef Stage<BR, BK, NT, KC> S;
#pragma unroll
  for (int i = 0; i < S::NV; i++) {
    const int idx = threadIdx.x + i * NT;
    const int run = idx / S::C4, c = idx % S::C4 * 4;
    float4 x = v[i];
    if constexpr (VEC) {
      const bool kv = k0 + (KC ? c : run) < K;
      x.x = kv ? x.x : 0.f; x.y = kv ? x.y : 0.f; x.z = kv ? x.z : 0.f; x.w = kv ? x.w : 0.f;
    }
    if (S::FULL || idx < S::TOTAL) *reinterpret_cast<float4 *>(lds + run * S::LD + c) = x;
  }
}
// LDS -> the operand fragments of T 32-row sub-tiles for 4 MFMA k-steps: this lane's row `row` (+ 32 per sub-tile) at k .. k + 3 of a
// staged tile with run stride LD.  KC: one 16-byte read; RC: four 4-byte reads of the same k's.
template <int T, int LD, bool KC>
__device__ __forceinline__ void read_frags(const float *s, int row, int k, float (&f)[T][4]) {
#pragma unroll
  for (int i = 0; i < T; i++) {
    if constexpr (KC) {
      const float4 t = *reinterpret_cast<const float4 *>(s + (row + i * 32) * LD + k);
      f[i][0] = t.x; f[i][1] = t.y; f[i][2] = t.z; f[i][3] = t.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++) f[i][j] = s[(k + j) * LD + row + i * 32];
    }
  }
}

// The epilogue of the 32-row tile: gemm_epilogue's outputs (gemm_common.h; its arithmetic, gemm_epilogue_value) element by element, the
// old C read inside the value and the old W behind the store of C, under the uniform conditions that ask for them.  The tile's products are
// short (the S-row recurrent ones: 16 workgroups, 10-20 us), and gemm_epilogue costs them 0.6-0.8 us: 32 x 2048 x 256 11.2 -> 12.0 us,
// 32 x 256 x 512 17.9 -> 18.6 us, so does any form that reads the old C in front of the value (profiles/gemm_f32_staged_timing.txt).
// C/D layout of the 32x32 MFMA: col = lane&31, row = (e&3) + 8*(e>>2) + 4*(lane>>5).
template <int TM, int TN>
__device__ __forceinline__ void epilogue_by_element(const GemmArgs &g, const f32x16 (&acc)[TM][TN], int row0, int col0, int l31, int lh) {
  const aslp_gemm_epilogue &ep = g.ep;
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int n = 0; n < TN; n++) {
      const int col = col0 + n * 32 + l31;
      if (col >= g.N) continue;
      const float bias = ep.bias ? ep.bias[col] : 0.0f;
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int row = row0 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        if (row >= g.M) continue;
        float *cp = g.C + (long)row * g.ldc + col;
        const float v = gemm_epilogue_value(g, acc[i][n][e], [&] { return g.beta != 0.0f ? (ep.c_src ? ep.c_src[(long)row * ep.ld_c_src + col] : *cp) : 0.0f; }, bias);
        *cp = v;
        if (ep.W) ep.W[(long)row * ep.ldw + col] = fmaf(ep.w_alpha, v, ep.W[(long)row * ep.ldw + col]);
        if (ep.act_out) {
          float a = ep.act == 1 ? sigmoid_ref(v) : ep.act == 2 ? tanh_ref(v) : ep.act == 3 ? fmaxf(v, 0.0f) : v;
          ep.act_out[(long)row * ep.ld_act + col] = a;
        }
      }
    }
}

// A_KC: op(A) rows are contiguous in k (transA == 0).  B_KC: op(B) columns are contiguous in k (transB == 1).
template <int BM, int BN, int BK, int WGM, int WGN, bool A_KC, bool B_KC, bool VEC>
__global__ void __launch_bounds__(64 * WGM * WGN) gemm_f32_mfma(GemmArgs g) {
  constexpr int NT = 64 * WGM * WGN;
  constexpr int WM = BM / WGM, WN = BN / WGN;  // wave patch
  constexpr int TM = WM / 32, TN = WN / 32;    // 32x32 MFMA tiles per wave
  static_assert((WGM * WGN == 4 || WGM * WGN == 8) && TM >= 1 && TN >= 1, "bad wave grid");
  typedef Stage<BM, BK, NT, A_KC> SA;
  typedef Stage<BN, BK, NT, B_KC> SB;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  // layout [A0 | B0 | A1 | B1]
  auto a_buf = [&](int b) { return lds + b * (SA::kFloats + SB::kFloats); };
  auto b_buf = [&](int b) { return lds + b * (SA::kFloats + SB::kFloats) + SA::kFloats; };

  int tm, tn;
  xcd_tile<BM, BN>(g, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave / WGN, wn = wave % WGN;
  const int l31 = lane & 31, lh = lane >> 5;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int j = 0; j < TN; j++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[i][j][e] = 0.0f;

  // two register stages: while tile t is multiplied out of LDS, tile t+1 sits in one stage
  // (already landed) and tile t+2 is in flight into the other -- >= one full MFMA phase of
  // latency slack for every global load.
  float4 ra0[SA::NV], rb0[SB::NV], ra1[SA::NV], rb1[SB::NV];
  auto load = [&](int kt, float4 (&ra)[SA::NV], float4 (&rb)[SB::NV]) {
    gload<BM, BK, NT, A_KC, VEC>(g.A, g.lda, g.M, g.K, m0, kt * BK, ra);
    gload<BN, BK, NT, B_KC, VEC>(g.B, g.ldb, g.N, g.K, n0, kt * BK, rb);
  };
  auto store = [&](int buf, int kt, const float4 (&ra)[SA::NV], const float4 (&rb)[SB::NV]) {
    sstore<BM, BK, NT, A_KC, VEC>(a_buf(buf), ra, kt * BK, g.K);
    sstore<BN, BK, NT, B_KC, VEC>(b_buf(buf), rb, kt * BK, g.K);
  };
  // the MFMAs of one K tile, its LDS reads interleaved: lane l takes k = 8 h + 4 (l >> 5) + {0..3} of row (l & 31)
  auto compute = [&](int cur) {
#pragma unroll
    for (int h = 0; h < BK / 8; h++) {
      float af[TM][4], bf[TN][4];
      read_frags<TM, SA::LD, A_KC>(a_buf(cur), wm * WM + l31, h * 8 + lh * 4, af);
      read_frags<TN, SB::LD, B_KC>(b_buf(cur), wn * WN + l31, h * 8 + lh * 4, bf);
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int i = 0; i < TM; i++)
#pragma unroll
          for (int n = 0; n < TN; n++)
            acc[i][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][j], bf[n][j], acc[i][n], 0, 0, 0);
    }
  };

  // Branch-free steady state: the k-tile count is rounded up to even (a tile beyond K loads from
  // clamped addresses and is zeroed at store time, so it adds 0), and loads/stores for tiles past
  // the end are issued unconditionally into buffers nobody reads.  With no conditional code
  // between the loads and their use the compiler keeps exact vmcnt counts: a store of stage X
  // waits only for stage X, the other stage's loads stay in flight across the barrier.
  const int ktiles = (g.K + BK - 1) / BK;
  const int kt_end = (ktiles + 1) & ~1;
  if (ktiles > 0) {
    load(0, ra0, rb0);
    store(0, 0, ra0, rb0);
    load(1, ra1, rb1);
  }
  __syncthreads();

  for (int kt = 0; kt < kt_end; kt += 2) {
    // even step: tile kt in LDS[0], tile kt+1 in stage 1 (landed), load kt+2 into stage 0
    load(kt + 2, ra0, rb0);
    __builtin_amdgcn_sched_barrier(0);  // keep the prefetch issue ABOVE the MFMA phase
    compute(0);
    __builtin_amdgcn_sched_barrier(0);
    store(1, kt + 1, ra1, rb1);
    __syncthreads();
    // odd step: tile kt+1 in LDS[1], tile kt+2 in stage 0, load kt+3 into stage 1
    load(kt + 3, ra1, rb1);
    __builtin_amdgcn_sched_barrier(0);
    compute(1);
    __builtin_amdgcn_sched_barrier(0);
    store(0, kt + 2, ra0, rb0);
    __syncthreads();
  }

  if constexpr (BM == 32) epilogue_by_element<TM, TN>(g, acc, m0 + wm * WM, n0 + wn * WN, l31, lh);
  else gemm_epilogue<TM, TN>(g, acc, m0 + wm * WM, n0 + wn * WN, l31, lh);
}

// aslp_gemm_epilogue.colstats by one pass over the finished C, for the kernels that do not form them in their epilogue
// (register-staged tiles): thread = column, blockIdx.y = 32-row group; the same three sums in the same per-group layout.
__global__ void __launch_bounds__(64) colstats_kernel(const float *__restrict__ C, int ldc, int M, int N, double *__restrict__ stats, int ld, int groups) {
  const int col = blockIdx.x * 64 + threadIdx.x, grp = blockIdx.y;
  if (col >= N) return;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  const int r1 = min(M, 32 * grp + 32);
  for (int r = 32 * grp; r < r1; r++) {
    const float v = C[(long)r * ldc + col];
    s0 += (double)v; s1 += (double)(v * v); s2 += (double)v * (double)v;
  }
  double *p = stats + (long)grp * ld + col;
  const long plane = (long)groups * ld;
  p[0] = s0; p[plane] = s1; p[2 * plane] = s2;
}

// ---- profile counters (bench.py roofline) -------------------------------------------------
struct GemmProf {
  long launches = 0;
  double flops = 0.0, ms = 0.0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
  std::vector<long> pending_shape;  // parallel to pending: (M << 40) | (N << 20) | K of the launch
  std::map<long, std::pair<long, double>> shape_ms;  // shape -> launches, milliseconds (aslp_gemm_profile_dump)
  std::map<int, double> cfg_flops;  // tile configuration actually launched -> flops it carried
};
GemmProf g_prof[4];
thread_local int t_last_cfg = 0;    // what launch_variant chose for the calling thread's latest product
bool g_prof_on = false;
std::mutex g_prof_mu;
std::vector<hipEvent_t> g_event_pool;  // recycled: no event creation / destruction inside a timed region

hipEvent_t take_event() {
  if (!g_event_pool.empty()) {
    hipEvent_t e = g_event_pool.back();
    g_event_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

void drain(GemmProf &p) {
  for (size_t i = 0; i < p.pending.size(); i++) {
    auto &ev = p.pending[i];
    float ms = 0.f;
    if (hipEventSynchronize(ev.second) == hipSuccess && hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) {
      p.ms += ms;
      auto &sh = p.shape_ms[p.pending_shape[i]];
      sh.first++;
      sh.second += ms;
    }
    g_event_pool.push_back(ev.first);
    g_event_pool.push_back(ev.second);
  }
  p.pending.clear();
  p.pending_shape.clear();
}

int g_force_tile = 0;  // aslp_gemm_force_tile: 0 = heuristic, else a tile of launch_variant (1, 7, 12) or of gemm_glds_launch (2xx) by number

// report order of aslp_gemm_profile_get and of the ASLP_GEMM_TILE_* hooks: 0 = NT, 1 = NN, 2 = TN, 3 = TT
int layout_slot(bool transA, bool transB) { return transA ? (transB ? 3 : 2) : (transB ? 0 : 1); }

template <int BM, int BN, int BK, int WGM, int WGN, bool A_KC, bool B_KC, bool VEC>
void launch_cfg(GemmArgs &g) {
  g.tiles_m = (g.M + BM - 1) / BM;
  g.tiles_n = (g.N + BN - 1) / BN;
  constexpr int NT = 64 * WGM * WGN;  // two LDS buffers of an A and a B tile
  constexpr int lds_bytes = 2 * (Stage<BM, BK, NT, A_KC>::kFloats + Stage<BN, BK, NT, B_KC>::kFloats) * (int)sizeof(float);
  auto kern = gemm_f32_mfma<BM, BN, BK, WGM, WGN, A_KC, B_KC, VEC>;
  static bool attr_set = false;  // one per template instantiation
  if (!attr_set) {
    if (lds_bytes > 48 * 1024)
      ASLP_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
    attr_set = true;
  }
  hipLaunchKernelGGL(kern, dim3(g.tiles_m * g.tiles_n), dim3(64 * WGM * WGN), lds_bytes, cur_stream(), g);
}

template <bool A_KC, bool B_KC, bool VEC>
void launch_variant(GemmArgs &g) {
  // Tile choice.  The heuristic names an LDS-DMA kernel (cfg >= 200, gemm_glds.hip), which takes the product if it is eligible:
  //   208  64 x 128 on 4 waves (32 x 64 per wave, half the fragment reads per MFMA): a weight-gradient product (neither operand
  //        K-contiguous) that tiles into >= 200 full 64 x 128 blocks.  After the epilogue rewrite 1 % ahead on cfg2 inside the training
  //        step (devtools/sweep_env.sh: 773.3 vs 781.7 k frames/s over three alternations, TN 74.5 vs 73.7 us), neutral on LC-BLSTM.
  //   212  64 x 128 on 8 waves: the other products with such a grid and one K-contiguous operand.
  //   207  64 x 64 on 4 waves, two or more workgroups per CU: everything else -- ragged edges, small grids, and every forward product
  //        (both operands K-contiguous), where it is 3 % ahead of 212 inside the training step (devtools/sweep_tiles.sh: 70.0 vs
  //        72.5 us average over the NT launches).
  // A product the LDS-DMA kernels decline (unaligned, a size that is no multiple of 4: DESIGN.md §7 "Sizes that are no multiple of 4")
  // runs on the register-staged kernel of this file with the same tile: 7 (64 x 64) for 207, 12 (64 x 128, 8 waves) for the others, and
  // 1 (32 x 128) for M <= 32, the S-row recurrent products of the LSTM family.  devtools/bench_gemm.py times any of them by number.
  // (32 x 64 / 32 x 128 tiles for products whose 64 x 64 grid leaves a third of the chip idle were measured on the LC-BLSTM step:
  //  1920 x 256 x 512 16.4 vs 17.1 us, but the long-K members lose their K split: 4.21 vs 3.75 ms per step.  Not taken.)
  auto blocks = [&](int bm, int bn) { return (long)((g.M + bm - 1) / bm) * ((g.N + bn - 1) / bn) * (g.pair ? 2 : 1); };
  int cfg;
  // experiment hook: ASLP_GEMM_TILE_{NT,NN,TN,TT}=<cfg> overrides the choice for one operand layout on a big grid
  static const int env_tile[4] = {getenv("ASLP_GEMM_TILE_NT") ? atoi(getenv("ASLP_GEMM_TILE_NT")) : 0, getenv("ASLP_GEMM_TILE_NN") ? atoi(getenv("ASLP_GEMM_TILE_NN")) : 0,
                                  getenv("ASLP_GEMM_TILE_TN") ? atoi(getenv("ASLP_GEMM_TILE_TN")) : 0, getenv("ASLP_GEMM_TILE_TT") ? atoi(getenv("ASLP_GEMM_TILE_TT")) : 0};
  const int env_cfg = env_tile[layout_slot(!A_KC, B_KC)];
  const bool big_grid = g.N % 128 == 0 && g.M % 64 == 0 && blocks(64, 128) >= 200;
  if (g_force_tile) cfg = g_force_tile;
  else if (env_cfg && big_grid) cfg = env_cfg;
  else if (big_grid && !A_KC && !B_KC) cfg = 208;
  else if (big_grid && !(A_KC && B_KC)) cfg = 212;
  else cfg = 207;
  t_last_cfg = cfg;
  if (cfg >= 200) {
    int used = cfg;
    if (gemm_glds_launch(g, A_KC, B_KC, cfg, &used)) {  // column sums / column statistics done in-kernel
      t_last_cfg = used;
      if (!A_KC) { g.ep.colsum = nullptr; g.ep1.colsum = nullptr; }
      g.ep.colstats = nullptr;
      return;
    }
    if (g.pair) { t_last_cfg = -1; return; }  // only the LDS-DMA kernels take pairs: the caller issues two single products
    if (cfg != 205 && cfg != 206 && cfg != 207 && cfg != 208 && cfg != 211 && cfg != 212 && cfg != 213) {
      set_error("aslp_sgemm: unknown tile configuration " + std::to_string(cfg) + " (ASLP_GEMM_TILE_* / aslp_gemm_force_tile)");
      return;
    }
    cfg = g.M <= 32 ? 1 : (cfg == 207 ? 7 : 12);  // not eligible: register-staged kernel of the same tile
    t_last_cfg = cfg;
  }
  if (g.pair) { t_last_cfg = -1; return; }
  switch (cfg) {
    case 1: launch_cfg<32, 128, 16, 1, 4, A_KC, B_KC, VEC>(g); break;
    case 7: launch_cfg<64, 64, 32, 2, 2, A_KC, B_KC, VEC>(g); break;
    case 12: launch_cfg<64, 128, 32, 2, 4, A_KC, B_KC, VEC>(g); break;   // 8 waves
    default: set_error("aslp_sgemm: unknown tile configuration " + std::to_string(cfg) + " (ASLP_GEMM_TILE_* / aslp_gemm_force_tile)"); break;
  }
}

template <bool A_KC, bool B_KC>
void launch_aligned(GemmArgs &g) {
  // vector path: 16-byte aligned operands whose contiguous extent is a multiple of 4 floats
  const int a_ext = A_KC ? g.K : g.M, b_ext = B_KC ? g.K : g.N;
  const bool vec = g.a_vec && g.b_vec && a_ext % 4 == 0 && b_ext % 4 == 0 && a_ext >= 4 && b_ext >= 4;
  if (vec) launch_variant<A_KC, B_KC, true>(g);
  else launch_variant<A_KC, B_KC, false>(g);
}

void launch_layout(GemmArgs &g, bool transA, bool transB) {
  if (!transA && transB) launch_aligned<true, true>(g);
  else if (!transA && !transB) launch_aligned<true, false>(g);
  else if (transA && !transB) launch_aligned<false, false>(g);
  else launch_aligned<false, true>(g);
}

// the arguments of one product, every optional piece off (no K split, no second product of a pair)
GemmArgs make_args(int M, int N, int K, float alpha, const float *A, int lda, const float *B, int ldb, float beta, float *C, int ldc,
                   const aslp_gemm_epilogue *ep) {
  static const int wide = [] { const char *e = getenv("ASLP_GEMM_WIDE_EPI"); return e ? atoi(e) : 1; }();
  GemmArgs g;
  g.A = A; g.B = B; g.C = C; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc;
  g.alpha = alpha; g.beta = beta;
  g.ep = ep ? *ep : aslp_gemm_epilogue();  // zero-initialised: every optional piece off
  g.a_vec = aligned16(A) && lda % 4 == 0;
  g.b_vec = aligned16(B) && ldb % 4 == 0;
  g.wide_epilogue = wide;
  g.tiles_m = g.tiles_n = 0;
  g.split_k = 0; g.k_chunk = 0; g.split_stride = 0;
  g.pair = 0; g.A1 = g.B1 = nullptr; g.C1 = nullptr; g.ep1 = aslp_gemm_epilogue();
  return g;
}

// `products` launched products of one shape on tile t_last_cfg go into the layout's counters; e0 / e1: the events around a timed one
void book_launch(int slot, int products, int M, int N, int K, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr) {
  const double flops = 2.0 * products * (double)M * (double)N * (double)K;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  GemmProf &p = g_prof[slot];
  p.launches += products;
  p.flops += flops;
  p.cfg_flops[t_last_cfg] += flops;
  if (e0) {
    (void)hipEventRecord(e1, cur_stream());
    p.pending.emplace_back(e0, e1);
    p.pending_shape.push_back(((long)M << 40) | ((long)N << 20) | (long)K);
  }
}

}  // namespace
}  // namespace aslp

using namespace aslp;

extern "C" {

// aslp_sgemm_ex with optional prepared planes of either operand (split16.h); an operand without planes is converted in scratch
static int sgemm_impl(int transA, int transB, int M, int N, int K, float alpha, const float *A, int lda, const float *B, int ldb, float beta,
                      float *C, int ldc, const aslp_gemm_epilogue *ep, const S16View *pa, const S16View *pb) {
  gemm_split16_reset_last_parts();
  if (M < 0 || N < 0 || K < 0) return -1;
  if (M == 0 || N == 0) return 0;
  if (!C || ldc < N) return -2;
  if (K > 0 && (!A || !B)) return -3;
  if (K > 0 && (lda < (transA ? M : K) || ldb < (transB ? K : N))) return -4;
  GemmArgs g = make_args(M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, ep);
  if (g.ep.colsum && !transA) return -5;  // column sums are defined for transposed A only
  if (g.ep.colstats && (beta != 0.0f || g.ep.W || g.ep.colstats_ld < N)) return -6;  // statistics of a plain forward product only
  if (g.ep.c_src && g.ep.ld_c_src < N) return -7;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  bool prof = g_prof_on;
  if (prof) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    e0 = take_event();
    e1 = take_event();
  }
  if (prof) (void)hipEventRecord(e0, cur_stream());
  static const int s16_cfg = [] { const char *e = getenv("ASLP_GEMM_SPLIT_F16_TILE"); return e ? atoi(e) : 0; }();
  if (gemm_split16_enabled() && !g_force_tile && gemm_split16_launch(g, !transA, transB != 0, s16_cfg, pa, pb)) {   // (a forced tile asks for an fp32 kernel by name)
    g.ep.colstats = nullptr;   // formed in its epilogue, like the column sums of a transposed A
    g.ep.colsum = nullptr;
    t_last_cfg = gemm_split16_last_tile();
  } else {
    g.ep.amax_parts = nullptr;   // the fp32 instruction's kernels leave no maxima of the activation output (aslp_gemm_last_parts() == 0)
    launch_layout(g, transA != 0, transB != 0);
  }
  if (g.ep.colstats) {  // the chosen kernel does not form them in its epilogue: one pass over the finished C
    const int groups = (M + 31) / 32;
    hipLaunchKernelGGL(colstats_kernel, dim3((N + 63) / 64, groups), dim3(64), 0, cur_stream(), C, ldc, M, N, g.ep.colstats, g.ep.colstats_ld, groups);
  }
  if (g.ep.colsum) {  // the chosen kernel could not fold the column sums in: one extra pass over A (same values)
    MatrixDim da = {K, M, lda};
    if (g.ep.colsum_w) aslp_add_row_sum_mat_vec_sgd(1.0f, A, da, g.ep.colsum_beta, g.ep.colsum, g.ep.colsum_w, g.ep.colsum_w_alpha);
    else aslp_add_row_sum_mat_vec(1.0f, A, da, g.ep.colsum_beta, g.ep.colsum);
  }
  check_launch("aslp_sgemm");
  book_launch(layout_slot(transA != 0, transB != 0), 1, M, N, K, e0, e1);
  return 0;
}

int aslp_sgemm_ex(int transA, int transB, int M, int N, int K, float alpha, const float *A, int lda, const float *B, int ldb, float beta,
                  float *C, int ldc, const aslp_gemm_epilogue *ep) {
  return sgemm_impl(transA, transB, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, ep, nullptr, nullptr);
}

// ---- prepared operand planes (include/aslp_kernels.h) ---------------------------------------------------------------------------
aslp_planes *aslp_planes_new(void) { return reinterpret_cast<aslp_planes *>(new PlaneSet()); }
void aslp_planes_free(aslp_planes *p) { delete reinterpret_cast<PlaneSet *>(p); }
int aslp_planes_convert(aslp_planes *p, const float *src, MatrixDim d) {
  if (!p || !src) return -1;
  const bool ok = reinterpret_cast<PlaneSet *>(p)->ConvertFrom(src, d.rows, d.cols, d.stride);
  check_launch("aslp_planes_convert");
  return ok ? 0 : -2;
}
int aslp_planes_convert_with_parts(aslp_planes *p, const float *src, MatrixDim d, int n_parts) {
  if (!p || !src || n_parts <= 0) return -1;
  PlaneSet *ps = reinterpret_cast<PlaneSet *>(p);
  if (!ps->Parts()) return -2;   // (the maxima were to be left in the set's own array)
  const bool ok = ps->ConvertWithParts(src, d.rows, d.cols, d.stride, n_parts);
  check_launch("aslp_planes_convert_with_parts");
  return ok ? 0 : -2;
}
void aslp_planes_reserve(aslp_planes *p, int rows, int cols) { if (p) reinterpret_cast<PlaneSet *>(p)->Reserve(rows, cols); }
void aslp_planes_set_bound(aslp_planes *p, float bound) { if (p) reinterpret_cast<PlaneSet *>(p)->SetBound(bound); }
void aslp_planes_as_output(const aslp_planes *p, aslp_planes_out *out) {
  if (!out) return;
  *out = aslp_planes_out();
  if (!p) return;
  const PlaneSet *ps = reinterpret_cast<const PlaneSet *>(p);
  const S16View v = ps->View();
  out->hi = v.hi; out->lo = v.lo; out->ld = v.ld; out->slot = v.slot; out->parts = ps->Parts(); out->nparts = 0; out->planes_written = 0;
}
int aslp_sgemm_planes_ex(int transA, int transB, int M, int N, int K, float alpha, const float *A, int lda, const aslp_planes *pa, const float *B,
                         int ldb, const aslp_planes *pb, float beta, float *C, int ldc, const aslp_gemm_epilogue *ep) {
  S16View va, vb;
  if (pa) va = reinterpret_cast<const PlaneSet *>(pa)->View();
  if (pb) vb = reinterpret_cast<const PlaneSet *>(pb)->View();
  return sgemm_impl(transA, transB, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, ep, pa ? &va : nullptr, pb ? &vb : nullptr);
}

// Two products of one shape in one launch (include/aslp_kernels.h).  Falls back to two launches wherever the paired kernel does
// not apply (unaligned operands, K % 4, column sums on a kernel that cannot fold them, the register-staged tiles).
int aslp_sgemm_pair_ex(int transA, int transB, int M, int N, int K, float alpha, const float *A0, const float *A1, int lda, const float *B0,
                       const float *B1, int ldb, float beta, float *C0, float *C1, int ldc, const aslp_gemm_epilogue *ep0,
                       const aslp_gemm_epilogue *ep1) {
  return aslp::sgemm_pair_views(transA, transB, M, N, K, alpha, A0, A1, lda, B0, B1, ldb, beta, C0, C1, ldc, ep0, ep1, nullptr, nullptr, nullptr, nullptr);
}
}  // extern "C"

// the pair with prepared planes (windows) of all four operands, or of none (csrc/split16.h)
int aslp::sgemm_pair_views(int transA, int transB, int M, int N, int K, float alpha, const float *A0, const float *A1, int lda, const float *B0,
                           const float *B1, int ldb, float beta, float *C0, float *C1, int ldc, const aslp_gemm_epilogue *ep0,
                           const aslp_gemm_epilogue *ep1, const S16View *va0, const S16View *va1, const S16View *vb0, const S16View *vb1) {
  static const int enabled = [] { const char *e = getenv("ASLP_GEMM_PAIR"); return e ? atoi(e) : 1; }();
  const bool views = va0 && va1 && vb0 && vb1;
  auto two = [&]() {
    const int rc = sgemm_impl(transA, transB, M, N, K, alpha, A0, lda, B0, ldb, beta, C0, ldc, ep0, views ? va0 : nullptr, views ? vb0 : nullptr);
    return rc ? rc : sgemm_impl(transA, transB, M, N, K, alpha, A1, lda, B1, ldb, beta, C1, ldc, ep1, views ? va1 : nullptr, views ? vb1 : nullptr);
  };
  if (M <= 0 || N <= 0 || K <= 0 || !A0 || !A1 || !B0 || !B1 || !C0 || !C1 || ldc < N) return two();  // argument errors are reported there
  if (lda < (transA ? M : K) || ldb < (transB ? K : N)) return two();
  const bool colsum = (ep0 && (ep0->colsum || ep0->colstats)) || (ep1 && (ep1->colsum || ep1->colstats));
  if (!enabled || g_prof_on || colsum) return two();   // per-launch event timing and the column-sum fallback work on single products
  GemmArgs g = make_args(M, N, K, alpha, A0, lda, B0, ldb, beta, C0, ldc, ep0);
  g.pair = 1; g.A1 = A1; g.B1 = B1; g.C1 = C1;
  g.ep1 = ep1 ? *ep1 : aslp_gemm_epilogue();
  g.a_vec = g.a_vec && aligned16(A1);
  g.b_vec = g.b_vec && aligned16(B1);
  if (!g.a_vec || !g.b_vec) return two();
  gemm_split16_reset_last_parts();
  if (views && gemm_split16_serves(M, N, K) && !g_force_tile && K % 64 == 0 &&
      gemm_split16_planes_launch(g, !transA, transB != 0, *va0, *vb0, va1, vb1, 0)) {
    t_last_cfg = gemm_split16_last_tile();
    check_launch("aslp_sgemm_pair (split-fp16)");
    book_launch(layout_slot(transA != 0, transB != 0), 2, M, N, K);
    return 0;
  }
  g.ep.amax_parts = g.ep1.amax_parts = nullptr;   // (as sgemm_impl)
  launch_layout(g, transA != 0, transB != 0);
  if (t_last_cfg < 0) return two();
  check_launch("aslp_sgemm_pair");
  book_launch(layout_slot(transA != 0, transB != 0), 2, M, N, K);
  return 0;
}

extern "C" {
int aslp_sgemm(int transA, int transB, int M, int N, int K, float alpha, const float *A, int lda, const float *B, int ldb, float beta,
               float *C, int ldc) {
  return aslp_sgemm_ex(transA, transB, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, nullptr);
}

void aslp_gemm_force_tile(int cfg) { g_force_tile = cfg; }
int aslp_gemm_last_tile(void) { return t_last_cfg; }
void aslp_gemm_profile(int enable) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof_on = enable != 0;
  if (g_prof_on)  // events for ~100 training steps up front, so the timed region only records
    while (g_event_pool.size() < 4096) {
      hipEvent_t e = nullptr;
      if (hipEventCreate(&e) != hipSuccess) break;
      g_event_pool.push_back(e);
    }
}
void aslp_gemm_profile_reset(void) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (auto &p : g_prof) {
    drain(p);
    p.launches = 0;
    p.flops = 0.0;
    p.ms = 0.0;
    p.cfg_flops.clear();
    p.shape_ms.clear();
  }
}
long aslp_gemm_profile_get(int variant, double *flops, double *ms) {
  if (variant < 0 || variant > 3) return -1;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  drain(g_prof[variant]);
  if (flops) *flops = g_prof[variant].flops;
  if (ms) *ms = g_prof[variant].ms;
  return g_prof[variant].launches;
}
void aslp_gemm_profile_dump(void) {  // devtools: per-shape table of the event-timed launches since the last reset, to stderr
  std::lock_guard<std::mutex> lk(g_prof_mu);
  const char *names[4] = {"NT", "NN", "TN", "TT"};
  for (int v = 0; v < 4; v++) {
    drain(g_prof[v]);
    for (auto &kv : g_prof[v].shape_ms) {
      const long M = kv.first >> 40, N = (kv.first >> 20) & 0xFFFFF, K = kv.first & 0xFFFFF;
      const double us = kv.second.second * 1e3 / kv.second.first;
      std::fprintf(stderr, "gemm %s %6ld x %6ld x %6ld  launches %5ld  avg %8.2f us  %7.1f TFLOP/s\n", names[v], M, N, K, kv.second.first, us,
                   2.0 * M * N * K / us / 1e6);
    }
  }
}
double aslp_gemm_profile_tile_flops(int variant, int tile_lo, int tile_hi) {
  if (variant < 0 || variant > 3) return 0.0;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  double fl = 0.0;
  for (auto &kv : g_prof[variant].cfg_flops)
    if (kv.first >= tile_lo && kv.first < tile_hi) fl += kv.second;
  return fl;
}
int aslp_gemm_profile_tile(int variant, char *buf, int buflen) {
  if (variant < 0 || variant > 3) return 0;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  int best = 0;
  double fl = -1.0;
  for (auto &kv : g_prof[variant].cfg_flops)
    if (kv.second > fl) { fl = kv.second; best = kv.first; }
  const char *d = "";
  switch (best) {  // the tables of launch_variant (register-staged) and gemm_glds_launch (LDS-DMA)
    case 1: d = "gemm_f32_mfma 32x128x16, 4 waves, register-staged"; break;
    case 7: d = "gemm_f32_mfma 64x64x32, 4 waves, register-staged"; break;
    case 12: d = "gemm_f32_mfma 64x128x32, 8 waves, register-staged"; break;
    case 205: d = "gemm_f32_glds 32x128x32, 4 waves, LDS-DMA, 4 stages"; break;
    case 206: d = "gemm_f32_glds 32x64x32, 2 waves, LDS-DMA, 4 stages"; break;
    case 207: d = "gemm_f32_glds 64x64x32, 4 waves, LDS-DMA, 4 stages"; break;
    case 208: d = "gemm_f32_glds 64x128x32, 4 waves, LDS-DMA, 3 stages"; break;
    case 211: d = "gemm_f32_glds 128x128x32, 8 waves, LDS-DMA, 3 stages"; break;
    case 212: d = "gemm_f32_glds 64x128x32, 8 waves, LDS-DMA, 3 stages"; break;
    case 213: d = "gemm_f32_glds 64x128x32, 8 waves, LDS-DMA, 4 stages"; break;
    case 304: d = "gemm_s16_glds 32x64x64 halves, 2 waves, v_mfma_f32_32x32x16_f16 x3 on two-piece fp32 operands, LDS-DMA, 3 stages"; break;
    case 308: d = "gemm_s16_glds 64x128x64 halves, 4 waves, v_mfma_f32_32x32x16_f16 x3 on two-piece fp32 operands, LDS-DMA, 3 stages"; break;
    case 311: d = "gemm_s16_glds 128x128x64 halves, 4 waves, v_mfma_f32_32x32x16_f16 x3 on two-piece fp32 operands, LDS-DMA, 2 stages"; break;
    case 351: d = "gemm_s16_pc 128x128x64 halves, 4 consumer + 4 producer waves, v_mfma_f32_32x32x16_f16 x3 on two-piece fp32 operands, LDS-DMA, 2 stages"; break;
    case 404: d = "gemm_s16_glds 32x64x64 halves, 2 waves, v_mfma_f32_32x32x16_f16 x1 on one-plane fp16 operands, LDS-DMA, 3 stages"; break;
    case 408: d = "gemm_s16_glds 64x128x64 halves, 4 waves, v_mfma_f32_32x32x16_f16 x1 on one-plane fp16 operands, LDS-DMA, 3 stages"; break;
    case 411: d = "gemm_s16_glds 128x128x64 halves, 4 waves, v_mfma_f32_32x32x16_f16 x1 on one-plane fp16 operands, LDS-DMA, 2 stages"; break;
    case 328: d = "gemm_s16_ks128 128x128x32 halves, 4 waves, v_mfma_f32_32x32x16_f16 x3 on two-piece fp32 operands, transposing LDS reads, ring of 4"; break;
    default: d = "gemm_f32_mfma (devtools tile)"; break;
  }
  if (buf && buflen > 0) { std::strncpy(buf, d, buflen - 1); buf[buflen - 1] = 0; }
  return best;
}

}  // extern "C"
