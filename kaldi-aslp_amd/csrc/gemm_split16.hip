// gemm_split16.hip -- fp32 GEMM carried on the fp16 matrix instruction (v_mfma_f32_32x32x16_f16) with fp32-equivalent operands.
//
// The fp32 MFMA rate of gfx950 is 256 FLOP/clk/CU (157 TFLOP/s) whatever the instruction shape; the fp16 instruction runs 16 x that.
// An fp32 value x is carried as TWO fp16 pieces behind a power-of-two scale s of its matrix (split16.h):  x s = hi + 2^-11 lo'.
// A product a b then is  hi_a hi_b + 2^-11 (hi_a lo'_b + lo'_a hi_b)  (+ 2^-22 lo'_a lo'_b, dropped: below the pieces' own rounding):
// three instructions per 16-wide k step, every partial product exact in the multiplier, accumulated in fp32 in two accumulators (main and
// cross terms) that are joined once in front of the epilogue.  Measured against double (tests/test_gemm_split16_gpu.py) the result is
// closer than the fp32 instruction's.
//
// Operands reach the kernel as PLANES in the layout of their matrix (split16.h): made once per tensor and step -- by the kernel that
// writes the tensor where that kernel knows a bound of it, else by split16_convert_kernel -- and read by every product the tensor
// takes part in, whichever index that product reduces over:
//   * reduction index contiguous ("KC": x in the forward product, dy in the in-diff, W in the forward product): LDS image
//     [rows][64 halves], 128-byte rows with gemm_glds.hip's chunk swizzle, fragments by ds_read_b128;
//   * reduction index = row index ("KS": dy and x in the weight gradient, W in the in-diff): LDS image [64 k][BR halves] exactly as the
//     rows lie in memory, fragments by TWO ds_read_b64_tr_b16 -- each 16-lane group reads a [4 k][16 columns] block and receives it
//     transposed, lane (column) p holding k .. k+3 (checked lane by lane on the device: devtools/micro/tr_read.hip).  The 64-byte
//     column groups of a k row are XOR-swizzled with the row's low bits so that the four rows a 32-lane group touches fall on four
//     different quarters of the 64 banks.
// Everything else is gemm_glds.hip's pipeline: LDS-DMA (global_load_lds_dwordx4) into NS stages, counted vmcnt, fragments double
// buffered in registers, the epilogues of gemm_common.h unchanged (the 32 x 32 fp16 instruction has the fp32 one's result layout).
//
// Where things live:
//   split16.h           the plane format (S16View, PlaneSet, the split itself)
//   gemm_s16_kernels.h  the product kernels gemm_s16_glds / gemm_s16_ks128 / gemm_s16_pc and the epilogue side they share
//   this file           the conversion kernels and PlaneSet, the launchers, the tile / split-K choice (s16_plan: a pure host function,
//                       exported as aslp_gemm_split16_plan) and the one switch that instantiates the kernels
//
// A/B: ASLP_GEMM_SPLIT_F16=0 keeps every product on the fp32 instruction (default: on).  ASLP_GEMM_S16_RAGGED=1 (default: off) also serves
// sizes that are no multiple of 4: the product kernels are the same, the conversion kernels take their RAGGED forms (gemm_split16_ragged below).
#include <algorithm>
#include <atomic>

#include "gemm_common.h"
#include "gemm_s16_kernels.h"
#include "scratch.h"
#include "split16.h"

namespace aslp {
namespace {

thread_local int t_last_cfg_s16 = 0;   // tile the calling thread's latest split-fp16 product ran on: 311 = 128x128, 351 = the same with producer / consumer waves, 308 = 64x128, 328 = 128x128 both operands reduction-major
thread_local int t_last_parts = 0;   // per-wave maxima the calling thread's latest product left (aslp_gemm_last_parts)

// ---- largest finite |x| of up to two matrices (blockIdx.y): every workgroup leaves its own maximum in part[workgroup] -- no atomics,
// nothing to zero first; the conversion reduces the partials.  Rows are dealt to the workgroups in contiguous chunks; a row is
// covered by tw = 2^tw_log2 threads with 16 bytes each per pass (no division anywhere, every load of a thread independent).
struct MaxJob { const float *p; int rows, cols, ld; float *part; };
struct MaxJobs { MaxJob j[kS16MaxJobs]; };
// RAGGED: some matrix of the launch has a width that is no multiple of 4 (the host chooses): the group that holds a row's last column
// is loaded column by column (split16.h s16_load4_ragged)
template <bool RAGGED>
__global__ void __launch_bounds__(256) s16_absmax_kernel(MaxJobs jobs, int tw_log2) {
  const MaxJob j = jobs.j[blockIdx.y];
  const int c4 = RAGGED ? (j.cols + 3) >> 2 : j.cols >> 2, tw = 1 << tw_log2, rpw = 256 >> tw_log2;
  const int tr = threadIdx.x >> tw_log2, tc = threadIdx.x & (tw - 1);
  const int per = (j.rows + gridDim.x - 1) / gridDim.x, r0 = blockIdx.x * per, r1 = min(j.rows, r0 + per);
  float m = 0.f;
  for (int r = r0 + tr; r < r1; r += rpw) {
    const float *row = j.p + (long)r * j.ld;
    if constexpr (RAGGED) {
#pragma unroll 4
      for (int c = tc; c < c4; c += tw) m = s16_absmax4(m, s16_load4_ragged(row, 4 * c, j.cols));
    } else {
#pragma unroll 4
      for (int c = tc; c < c4; c += tw) m = s16_absmax4(m, *reinterpret_cast<const float4 *>(row + 4 * c));
    }
  }
  m = wave_max(m);
  __shared__ float wm[4];
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) j.part[blockIdx.x] = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
}
// the matrix maximum from the partials (every thread of a 256-thread workgroup gets it)
__device__ __forceinline__ float reduce_parts(const float *part, int nparts) {
  __shared__ float wm2[4];
  float m = 0.f;
  for (int i = threadIdx.x; i < nparts; i += 256) m = fmaxf(m, part[i]);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) wm2[threadIdx.x >> 6] = m;
  __syncthreads();
  const float r = fmaxf(fmaxf(wm2[0], wm2[1]), fmaxf(wm2[2], wm2[3]));
  __syncthreads();   // (wm2 may be reused by a second reduction)
  return r;
}

// ---- bound of the weights after the next fused step (include/aslp_kernels.h aslp_weight_bound): one workgroup
struct BoundJob { const float *w_parts; int n_w; const float *c_parts; int n_c; const unsigned *slot_a, *slot_b; float k, alpha, beta, w_alpha, clip; unsigned *slot_out; };
__global__ void __launch_bounds__(256) s16_weight_bound_kernel(BoundJob j) {
  const float mw = reduce_parts(j.w_parts, j.n_w);
  const float mc = j.n_c > 0 ? reduce_parts(j.c_parts, j.n_c) : 0.f;
  if (threadIdx.x == 0) {
    const float ba = __uint_as_float(*j.slot_a), bb = __uint_as_float(*j.slot_b);
    float v = fabsf(j.alpha) * j.k * ba * bb + fabsf(j.beta) * mc;    // |alpha A^T B + beta C_old| <= alpha K max|a| max|b| + beta max|C_old|
    if (j.clip > 0.f) v = fminf(v, j.clip);
    *j.slot_out = __float_as_uint(mw + fabsf(j.w_alpha) * v);
  }
}

// ---- fp32 matrix -> planes in the matrix' own layout (padding written as zeros), up to two matrices per launch (blockIdx.y) --------
// Same dealing of rows; a thread converts 8 consecutive columns per pass (two 16-byte loads, one 16-byte store per plane).
struct ConvJob { const float *src; int ld_src; S16View pl; const float *part; int nparts; };
struct ConvJobs { ConvJob j[kS16MaxJobs]; };
// RAGGED: as s16_absmax_kernel -- in both branches the 4-column group that holds a row's last column takes the masked loads, so that the
// planes get zeros from column `cols` on and nothing from behind the matrix reaches them
template <bool RAGGED>
__global__ void __launch_bounds__(256) split16_convert_kernel(ConvJobs jobs, int tw_log2) {
  const ConvJob j = jobs.j[blockIdx.y];
  const int k8 = j.pl.ld >> 3, tw = 1 << tw_log2, rpw = 256 >> tw_log2;   // ld is a multiple of 64
  const int tr = threadIdx.x >> tw_log2, tc = threadIdx.x & (tw - 1);
  const int rows_p = (j.pl.rows + kS16Pad - 1) / kS16Pad * kS16Pad;
  const int per = (rows_p + gridDim.x - 1) / gridDim.x, r0 = blockIdx.x * per, r1 = min(rows_p, r0 + per);
  // A workgroup's share of a minibatch-sized matrix is a few 8-column pieces per thread: their loads go out before the maximum is read, so
  // the kernel is one round trip to memory deep instead of one for the partial maxima and one per row pass.
  constexpr int kPre = 4;
  const int units = max(r1 - r0, 0) * k8;
  if (units <= kPre * 256) {
    float4 a[kPre][2];
#pragma unroll
    for (int i = 0; i < kPre; i++) {
      const int u = (int)threadIdx.x + i * 256, ur = u / k8, r = r0 + ur, c = u - ur * k8;
      const bool ok = u < units && r < j.pl.rows;
      const float *row = j.src + (long)r * j.ld_src;
      if constexpr (RAGGED) {
        a[i][0] = ok && 8 * c < j.pl.cols ? s16_load4_ragged(row, 8 * c, j.pl.cols) : float4{0.f, 0.f, 0.f, 0.f};
        a[i][1] = ok && 8 * c + 4 < j.pl.cols ? s16_load4_ragged(row, 8 * c + 4, j.pl.cols) : float4{0.f, 0.f, 0.f, 0.f};
      } else {
        a[i][0] = ok && 8 * c < j.pl.cols ? *reinterpret_cast<const float4 *>(row + 8 * c) : float4{0.f, 0.f, 0.f, 0.f};
        a[i][1] = ok && 8 * c + 4 < j.pl.cols ? *reinterpret_cast<const float4 *>(row + 8 * c + 4) : float4{0.f, 0.f, 0.f, 0.f};
      }
    }
    const unsigned mbits = __float_as_uint(reduce_parts(j.part, j.nparts));
    if (blockIdx.x == 0 && threadIdx.x == 0) *j.pl.slot = mbits;
    const float s = ldexpf(1.f, s16_exponent(mbits));
#pragma unroll
    for (int i = 0; i < kPre; i++) {
      const int u = (int)threadIdx.x + i * 256, ur = u / k8, r = r0 + ur, c = u - ur * k8;
      if (u >= units) break;
      half4 h0, l0, h1, l1;
      s16_split4(a[i][0], s, &h0, &l0);   // (padding: zeros split into zeros)
      s16_split4(a[i][1], s, &h1, &l1);
      *reinterpret_cast<half8 *>(j.pl.hi + (long)r * j.pl.ld + 8 * c) = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
      *reinterpret_cast<half8 *>(j.pl.lo + (long)r * j.pl.ld + 8 * c) = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
    }
    return;
  }
  const unsigned mbits = __float_as_uint(reduce_parts(j.part, j.nparts));
  if (blockIdx.x == 0 && threadIdx.x == 0) *j.pl.slot = mbits;   // for the products (launched behind this kernel)
  const float s = ldexpf(1.f, s16_exponent(mbits));
  for (int r = r0 + tr; r < r1; r += rpw) {
    const float *row = j.src + (long)r * j.ld_src;
    const bool row_ok = r < j.pl.rows;
#pragma unroll 2
    for (int c = tc; c < k8; c += tw) {
      half4 h0 = {0, 0, 0, 0}, l0 = {0, 0, 0, 0}, h1 = {0, 0, 0, 0}, l1 = {0, 0, 0, 0};
      if constexpr (RAGGED) {
        if (row_ok && 8 * c < j.pl.cols) s16_split4(s16_load4_ragged(row, 8 * c, j.pl.cols), s, &h0, &l0);
        if (row_ok && 8 * c + 4 < j.pl.cols) s16_split4(s16_load4_ragged(row, 8 * c + 4, j.pl.cols), s, &h1, &l1);
      } else {
        if (row_ok && 8 * c < j.pl.cols) s16_split4(*reinterpret_cast<const float4 *>(row + 8 * c), s, &h0, &l0);          // cols % 4 == 0
        if (row_ok && 8 * c + 4 < j.pl.cols) s16_split4(*reinterpret_cast<const float4 *>(row + 8 * c + 4), s, &h1, &l1);
      }
      *reinterpret_cast<half8 *>(j.pl.hi + (long)r * j.pl.ld + 8 * c) = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
      *reinterpret_cast<half8 *>(j.pl.lo + (long)r * j.pl.ld + 8 * c) = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
    }
  }
}
// threads per row for `units` 16-byte (absmax) / 32-byte (convert) pieces per row
inline int tw_log2_for(int units) {
  int l = 0;
  while (l < 8 && (1 << l) < units) l++;
  return l;
}
// The launches of the two kernels for the first n jobs (matrices in one launch share the threads-per-row choice: the widest one's).  The
// ragged forms run only where a matrix of the launch has a width that is no multiple of 4; whether such a matrix may come here at all
// (gemm_split16_ragged) is the callers' business.
void launch_absmax(const MaxJobs &ms, int n) {
  int c4 = 0;
  bool ragged = false;
  for (int i = 0; i < n; i++) { c4 = std::max(c4, (ms.j[i].cols + 3) >> 2); ragged = ragged || (ms.j[i].cols & 3); }
  if (ragged) hipLaunchKernelGGL(s16_absmax_kernel<true>, dim3(kS16ConvParts, n), dim3(256), 0, cur_stream(), ms, tw_log2_for(c4));
  else hipLaunchKernelGGL(s16_absmax_kernel<false>, dim3(kS16ConvParts, n), dim3(256), 0, cur_stream(), ms, tw_log2_for(c4));
}
void launch_convert(const ConvJobs &js, int n, int grid_x) {
  int k8 = 0;
  bool ragged = false;
  for (int i = 0; i < n; i++) { k8 = std::max(k8, js.j[i].pl.ld >> 3); ragged = ragged || (js.j[i].pl.cols & 3); }
  if (ragged) hipLaunchKernelGGL(split16_convert_kernel<true>, dim3(grid_x, n), dim3(256), 0, cur_stream(), js, tw_log2_for(k8));
  else hipLaunchKernelGGL(split16_convert_kernel<false>, dim3(grid_x, n), dim3(256), 0, cur_stream(), js, tw_log2_for(k8));
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------------
// grid of BM x BN tiles (y: K chunks, z: the two products of a pair), the kernel's LDS allowance (once), the launch
template <auto KERN, int BM, int BN, int THREADS, int LDS_BYTES, bool EXTRA>
void s16_launch_tiles(GemmArgs &g, const S16Operands &ops) {
  g.tiles_m = (g.M + BM - 1) / BM;
  g.tiles_n = (g.N + BN - 1) / BN;
  static bool attr_set = false;
  if (!attr_set) {
    if (LDS_BYTES > 48 * 1024)
      ASLP_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
    attr_set = true;
  }
  hipLaunchKernelGGL(KERN, dim3(g.tiles_m * g.tiles_n, g.split_k > 1 ? g.split_k : 1, g.pair ? 2 : 1), dim3(THREADS), LDS_BYTES, cur_stream(), g, ops);
  t_last_parts = EXTRA ? g.tiles_m * g.tiles_n * (g.pair ? 2 : 1) : 0;
}
template <int BM, int BN, int KT, int NS, bool A_KC, bool B_KC, bool EXTRA, int ABL = 0>
void launch_s16_pc(GemmArgs &g, const S16Operands &ops) {
  s16_launch_tiles<gemm_s16_pc<BM, BN, KT, NS, A_KC, B_KC, EXTRA, ABL>, BM, BN, 512, NS * 4 * (BM + BN) * KT, EXTRA>(g, ops);
}
template <bool EXTRA>
void launch_s16_ks128(GemmArgs &g, const S16Operands &ops) {
  s16_launch_tiles<gemm_s16_ks128<EXTRA>, 128, 128, 256, 4 * 4 * 32 * 128 * 2, EXTRA>(g, ops);   // 128 KB
}
template <int BM, int BN, int WGM, int WGN, int NS, bool A_KC, bool B_KC, int ABL = 0, bool EXTRA = false, int NP = 2>
void launch_s16(GemmArgs &g, const S16Operands &ops) {
  s16_launch_tiles<gemm_s16_glds<BM, BN, WGM, WGN, NS, A_KC, B_KC, ABL, EXTRA, NP>, BM, BN, 64 * WGM * WGN, NS * NP * (BM + BN) * 128, EXTRA>(g, ops);
}

// ---- the choice ------------------------------------------------------------------------------------------------------------------------
// A/B switches and tuning aids of the choice, read from the environment once
struct S16Tuning {
  int ks128;            // ASLP_GEMM_KS128 (A/B switch, default 1): 0 = never the 128 x 128 kernel for two reduction-major operands
  double ks128_cost;    // ASLP_GEMM_KS128_COST (tuning aid, default 1.6): cost of a 128 x 128 round of that kernel in 64 x 128 rounds
  int any128;           // ASLP_GEMM_S16_128_ANY (tuning aid, default 0): 1 = 128 x 128 on every grid of >= 224 tiles, 2 = never
  int pc;               // ASLP_GEMM_S16_PC (A/B switch, default 1): 0 keeps the one-role kernel where the 128 x 128 tile was chosen
  int splitk;           // ASLP_GEMM_SPLITK (default 1): 0 = no split over K
  int small;            // ASLP_GEMM_S16_SMALL (A/B switch, default 1): 0 = no 32 x 64 tiles for minibatch-sized outputs
  int small_mink;       // ASLP_GEMM_S16_SMALL_MINK (tuning aid, default 256): smallest K for those tiles when planes / maxima are to be left
};
const S16Tuning &s16_tuning() {
  static const S16Tuning t = [] {
    auto num = [](const char *name, double dflt) { const char *e = getenv(name); return e ? atof(e) : dflt; };
    S16Tuning v;
    v.ks128 = (int)num("ASLP_GEMM_KS128", 1);
    v.ks128_cost = num("ASLP_GEMM_KS128_COST", 1.6);
    v.any128 = (int)num("ASLP_GEMM_S16_128_ANY", 0);
    v.pc = (int)num("ASLP_GEMM_S16_PC", 1);
    v.splitk = (int)num("ASLP_GEMM_SPLITK", 1) != 0;
    v.small = (int)num("ASLP_GEMM_S16_SMALL", 1) != 0;
    v.small_mink = (int)num("ASLP_GEMM_S16_SMALL_MINK", 256);
    return v;
  }();
  return t;
}
// what one epilogue asks the product to leave behind, and whether the 16-byte epilogue applies to it
struct S16Asks { int planes_of = 0; bool wmax = false, cmax = false, amax = false, colstats = false, colsum = false, wide_ok = false; };
// the decision.  tile: 304 = 32 x 64, 305 = the same with four stages (tuning aid), 308 = 64 x 128, 311 = 128 x 128 (gemm_s16_glds),
// 328 = 128 x 128 both operands reduction-major (gemm_s16_ks128), 351 = 128 x 128 with producer / consumer waves (gemm_s16_pc); one-plane
// products 404 / 408 / 411; 0 = not served.  split_k > 1: K in chunks of k_chunk over blockIdx.y on tile 308 / 408 with emptied epilogues,
// gemm_glds.hip's second launch adds the chunks and runs the epilogue.  drop_*: requests the launch must take out of the epilogues first.
struct S16Plan { int tile; int split_k; int k_chunk; bool drop_extras, drop_extras1, drop_maxima; };

// Tile for one launch (no split) of a product whose epilogues leave planes / maxima (`extra`) or not; cfg: a tile asked for by its
// two-plane number, 0 = choose.  t128 / t64: workgroups of 128 x 128 / 64 x 128 tiles.
int s16_plan_tile(bool a_kc, bool b_kc, int M, int N, bool extra, long t128, long t64, int planes, int cfg, const S16Tuning &tu) {
  const bool kc_kc = a_kc && b_kc;
  if (planes == 1) {
    // One-plane products (aslp_gemm_operand_planes(1)): the same three tiles of gemm_s16_glds reading the hi planes alone, reported as the
    // two-plane number + 100.  cfg names a tile by either number; the grid-fill reasoning is the two-plane one below, with the 128 x 128 threshold measured anew.
    // gemm_s16_ks128 and gemm_s16_pc have no one-plane form: where two planes would run them, one plane runs 408 / 411.
    if (cfg != 304 && cfg != 308 && !((cfg == 311 || cfg == 312 || cfg == 351) && kc_kc && !extra)) {
      // 128 x 128 from two full rounds of 256 workgroups on: with one plane the 64 x 128 tile runs two workgroups per CU (72 KB of LDS), so up to
      // 512 of them are one round -- measured 2048^3 27.0 (408) against 31.9 us (411), 4096 x 2048 x 2048 48.9 against 40.8, 4096^3 173 against
      // 137 (devtools/bench_gemm_planes.py); grids between 256 and 512 tiles of 128 x 128 were not measured and stay on the 64 x 128 tile
      cfg = (!extra && kc_kc && t128 >= 512 && 2 * ((t128 + 255) / 256) <= (t64 + 255) / 256) ? 311 : 308;
    }
    return cfg == 304 ? 404 : cfg == 308 ? 408 : 411;
  }
  // 128 x 128 where that still gives every CU a workgroup, else 64 x 128 (measured: 1024 x 2048 x 2048 52 against 70 us per call).  Only with
  // both operands reduction-contiguous: the transposing reads' address registers push the 128 x 128 tile past 512 registers (27-31 spilled),
  // and a kernel with a private segment pays ~1 ms per launch for it on this runtime.
  if (!a_kc && !b_kc) {
    // both operands reduction-major: the 128 x 128 kernel wherever its grid fills the chip about as well as the 64 x 128 one's --
    // rounds of 256 workgroups, a 128 x 128 round costing ~1.6 of a 64 x 128 one (measured on 2048 x 2048 x 1024)
    const double cost128 = tu.ks128_cost * (double)((t128 + 255) / 256), cost64 = (double)((t64 + 255) / 256);
    // (M and N multiples of 8 is what the kernel was measured and shipped with, and multiples of 4 keep that condition.  Nothing in the kernel
    // needs it -- the planes' pitch is a multiple of 64 halves, so every 16-byte piece it fetches is whole -- so an M or N that is no multiple
    // of 4, which gets here only under gemm_split16_ragged(), is taken like a multiple of 8)
    if (tu.ks128 && (cfg == 0 || cfg == 328) && (cfg == 328 || (t128 >= 200 && cost128 <= cost64)) && (((N % 8) == 0 && (M % 8) == 0) || ((M | N) & 3)))
      return 328;
  }
  // 128 x 128 (cfg 311; both operands reduction-contiguous, nothing extra to leave) where its rounds of 256 workgroups cost no more than the
  // 64 x 128 tile's, a 128 x 128 round counted as two: level at 2048^3 ... 8192 x 2048 x 2048 (57.8 / 222.3 against 57.4 / 220.8 us from
  // prepared planes), 1 % ahead at 4096^3, and inside the LC-BLSTM step, whose layer products come as pairs of 1920 x 2048 (480 against 960
  // workgroups), worth 2.87 against 2.93-3.05 ms; not where it leaves a ragged last round (1920 x 3000 x 1024: 58.1 against 48.5 us)
  if (cfg != 304 && cfg != 305 && (cfg == 0 || !kc_kc || extra))   // (311 / 312 / 351 asked for by number stand when the product is KC / KC without extras)
    cfg = (!extra && kc_kc && t128 >= 224 && tu.any128 != 2 && (tu.any128 == 1 || 2 * ((t128 + 255) / 256) <= (t64 + 255) / 256)) ? 311 : 308;
  // (Below 224 tiles -- cfg2's output layer, 1024 x 3000 x 2048: 192 workgroups of 128 x 128 in one round against 384 of 64 x 128 in two -- the
  // producer / consumer kernel wins only from operands that are hot in the L2: 66.5 against 74.2 us per call in a loop over one product,
  // 59.6 against 57.8 us inside the training step, where the weights' planes come from HBM and two stages hide less of that than three;
  // cfg2 0.756 against 0.754 ms per step, three alternations.  The floor stays.)
  // the producer / consumer kernel (gemm_s16_pc) where the 128 x 128 tile was chosen: 4096^3 383 against 422 us, same bits (devtools/micro/s16_pc.hip,
  // profiles/r06_gemm_s16_pc_micro.txt); ASLP_GEMM_S16_PC=0 keeps the one-role kernel (A/B switch)
  if (cfg == 311 && tu.pc) return 351;
  if (cfg == 312) return 311;   // (forced: the one-role kernel whatever the switch says)
  if (cfg == 305) return a_kc && !extra ? 305 : 0;   // (tuning aid: 32 x 64 with four stages)
  return (cfg == 304 || cfg == 308 || cfg == 311 || (cfg == 351 && kc_kc)) ? cfg : 0;
}

// The whole choice for a product of planes: tile, split over K and the requests that cannot be honoured.  Launches nothing.
S16Plan s16_plan(int M, int N, int K, bool a_kc, bool b_kc, bool pair, S16Asks ep, S16Asks ep1, int planes, int cfg, const S16Tuning &tu) {
  S16Plan p = {0, 0, 0, false, false, false};
  if (M < 64 || N < 64 || K < 32) return p;
  if (planes == 1 && cfg >= 400) cfg -= 100;   // (a one-plane tile asked for by its own number: the choices below speak in two-plane numbers)
  const int np = pair ? 2 : 1, kp = (K + BKH - 1) / BKH * BKH;
  if (!pair) ep1 = S16Asks();
  // planes / maxima of the output are written by the 16-byte epilogue only: where that does not apply the request is dropped (the
  // caller sees aslp_gemm_last_parts() == 0 and converts for itself)
  auto drop_extras = [](S16Asks &e) { e.planes_of = 0; e.wmax = e.cmax = e.amax = false; };
  p.drop_extras = !ep.wide_ok;
  p.drop_extras1 = pair && !ep1.wide_ok;
  if (p.drop_extras) drop_extras(ep);
  if (p.drop_extras1) drop_extras(ep1);
  // A long reduction on a grid that cannot fill the chip (the minibatch-256 layer products: 64 tiles of 64 x 128 for 256 CUs): K is split
  // over blockIdx.y, the chunks' partial products are added in chunk order by gemm_glds.hip's second launch, which also runs the epilogue
  // (bias, clip, SGD step, activation output -- not planes / maxima / column statistics: such requests keep the single launch).
  const long tiles = (long)((M + 63) / 64) * ((N + 127) / 128) * np, t128 = (long)((M + 127) / 128) * ((N + 127) / 128) * np;
  // per-workgroup maxima go to arrays of kS16MaxParts floats (PlaneSet::Parts, the components' own): a grid with more workgroups than
  // that leaves none (the smallest tile of such a grid is 64 x 128), and planes of updated weights, whose bound is formed from maxima, go too
  p.drop_maxima = tiles > kS16MaxParts;
  if (p.drop_maxima) {
    auto drop_maxima = [](S16Asks &e) { if (e.planes_of == 1) e.planes_of = 0; e.wmax = e.cmax = e.amax = false; };
    drop_maxima(ep);
    drop_maxima(ep1);
  }
  const bool leaves = ep.planes_of != 0 || ep.wmax || ep.cmax || ep.amax, leaves1 = ep1.planes_of != 0 || ep1.wmax || ep1.cmax || ep1.amax;
  const bool extras = leaves || ep.colstats || ep.colsum || leaves1 || ep1.colstats || ep1.colsum;
  // (act_out planes asked for by a forward product are given up for the split: the consumer converts the small activation matrix itself)
  // (the second launch writes the planes of an activation output and the maxima of |C| and of |act_out| itself: those requests go with the split)
  const bool reduce_serves = !ep.wmax && !ep.colstats && !ep.colsum && ep.planes_of != 1 && !pair;
  // ... unless 32 x 64 tiles fill the chip in ONE round with the whole reduction (256 x 2048 outputs: 15.2 us against 19.4 us for the
  // two launches of the split; the epilogue, with whatever it was asked to leave, stays in the product's launch)
  const long t32 = (long)((M + 31) / 32) * ((N + 63) / 64) * np;
  // (with planes / maxima to leave, from K = 256: there the 64 x 128 tile's launch, 64 workgroups each with a long epilogue, is the slower
  // one -- the 440-input layer of the minibatch-256 net 18.6 against 25.7 us; a plain product of that shape is faster on 64 x 128: 9.7 / 12.6)
  if (tu.small && cfg == 0 && tiles <= 64 && t32 <= 256 && K >= (leaves ? tu.small_mink : 1024)) cfg = 304;
  else if (tu.splitk && (!extras || reduce_serves) && (cfg == 0 || cfg == 308) && tiles <= 128 && K >= 1024) {
    int split = (int)(256 / tiles);
    if (split > K / 256) split = K / 256;
    if (split > 8) split = 8;
    const int chunk = ((kp / BKH + split - 1) / split) * BKH;
    split = (kp + chunk - 1) / chunk;
    if (split >= 2) {
      p.tile = planes == 1 ? 408 : 308;
      p.split_k = split;
      p.k_chunk = chunk;
      return p;
    }
  }
  p.tile = s16_plan_tile(a_kc, b_kc, M, N, leaves || leaves1, t128, tiles, planes, cfg, tu);
  return p;
}

// the kernel of a tile: every instantiation of the product kernels in the library is named here
template <bool A_KC, bool B_KC>
void s16_launch_tile(GemmArgs &g, const S16Operands &ops, int tile, bool extra) {
  switch (tile) {
    case 304:   // 32 x 64, two waves: 256 workgroups for a 256 x 2048 output with the whole reduction in one launch
      if (extra) launch_s16<32, 64, 1, 2, 3, A_KC, B_KC, 0, true>(g, ops);
      else launch_s16<32, 64, 1, 2, 3, A_KC, B_KC>(g, ops);
      break;
    case 305:
      if constexpr (A_KC) launch_s16<32, 64, 1, 2, 4, A_KC, B_KC>(g, ops);
      break;
    case 308:
      if (extra) launch_s16<64, 128, 2, 2, 3, A_KC, B_KC, 0, true>(g, ops);
      else launch_s16<64, 128, 2, 2, 3, A_KC, B_KC>(g, ops);
      break;
    case 311: if constexpr (A_KC && B_KC) launch_s16<128, 128, 2, 2, 2, true, true>(g, ops); break;
    case 328:
      if constexpr (!A_KC && !B_KC) { if (extra) launch_s16_ks128<true>(g, ops); else launch_s16_ks128<false>(g, ops); }
      break;
    case 351: if constexpr (A_KC && B_KC) launch_s16_pc<128, 128, 64, 2, true, true, false>(g, ops); break;
    case 404:
      if (extra) launch_s16<32, 64, 1, 2, 3, A_KC, B_KC, 0, true, 1>(g, ops);
      else launch_s16<32, 64, 1, 2, 3, A_KC, B_KC, 0, false, 1>(g, ops);
      break;
    case 408:
      if (extra) launch_s16<64, 128, 2, 2, 3, A_KC, B_KC, 0, true, 1>(g, ops);
      else launch_s16<64, 128, 2, 2, 3, A_KC, B_KC, 0, false, 1>(g, ops);
      break;
    case 411: if constexpr (A_KC && B_KC) launch_s16<128, 128, 2, 2, 2, true, true, 0, false, 1>(g, ops); break;
  }
}


int g_split16_override = -1;   // aslp_gemm_split16(): -1 = the environment decides
int g_split16_tile_override = -1;   // aslp_gemm_split16_tile(): -1 = ASLP_GEMM_SPLIT_F16_TILE / the heuristic
int g_operand_planes_override = -1;   // aslp_gemm_operand_planes(): -1 = ASLP_GEMM_PLANES decides
int g_ragged_override = -1;   // aslp_gemm_split16_ragged(): -1 = ASLP_GEMM_S16_RAGGED decides

}  // namespace

bool gemm_split16_enabled() {
  static const bool on = !(getenv("ASLP_GEMM_SPLIT_F16") != nullptr && getenv("ASLP_GEMM_SPLIT_F16")[0] == '0');
  return g_split16_override >= 0 ? g_split16_override != 0 : on;
}

// planes the products read per operand: 2 (default) or 1 = the hi planes alone (ASLP_GEMM_PLANES, aslp_gemm_operand_planes)
int gemm_operand_planes() {
  static const int env = [] { const char *e = getenv("ASLP_GEMM_PLANES"); return e == nullptr ? 0 : atoi(e); }();   // 1 or 2 count as a choice
  if (g_operand_planes_override > 0) return g_operand_planes_override;
  if (env == 1 || env == 2) return env;
  return fp16_operands_on() ? 1 : 2;
}

int s16_plane_ld(int cols) {
  // (an extra pitch of 64 or 128 halves on rows whose pitch is a multiple of 2 KB was measured: no effect on the layer products, 31.5 /
  //  31.6 / 31.8 us)
  return (cols + kS16Pad - 1) / kS16Pad * kS16Pad;
}
// Sizes that are no multiple of 4 (ASLP_GEMM_S16_RAGGED=1 / aslp_gemm_split16_ragged(1); default off, only "1" turns it on): the number
// of pdfs of a tree, 39 x 11 input widths, an utterance's frame count.  The product kernels never needed the multiple -- planes are padded
// to 64 both ways with zeros, the K loop runs over the padded extent, the narrow epilogue masks element by element -- the conversion
// kernels did, and have ragged forms now.  Not under the aslp_fp16_operands umbrella; works with either plane count.
bool gemm_split16_ragged() {
  static const bool env = [] { const char *e = getenv("ASLP_GEMM_S16_RAGGED"); return e != nullptr && e[0] == '1' && e[1] == '\0'; }();
  return g_ragged_override >= 0 ? g_ragged_override != 0 : env;
}
bool gemm_split16_serves(int M, int N, int K) {
  return gemm_split16_enabled() && M >= 128 && N >= 128 && K >= 64 && (gemm_split16_ragged() || !((M | N | K) & 3));
}
static int g_keep_override = -1;
bool s16_keep_weight_planes() {
  static const bool on = !(getenv("ASLP_KEEP_WEIGHT_PLANES") != nullptr && getenv("ASLP_KEEP_WEIGHT_PLANES")[0] == '0');
  return g_keep_override >= 0 ? g_keep_override != 0 : on;
}
static std::atomic<long> g_param_epoch{1};
long s16_param_epoch() { return g_param_epoch.load(std::memory_order_relaxed); }
long s16_new_epoch() {
  static std::atomic<long> counter{0};
  return ++counter;
}
S16DiffTarget &s16_loss_diff_target() {
  static thread_local S16DiffTarget t;
  return t;
}
S16Epochs &s16_epochs() {
  static thread_local S16Epochs e;
  return e;
}

// ---- PlaneSet ----------------------------------------------------------------------------------------------------------------------
PlaneSet::~PlaneSet() {
  // (process teardown may already have unloaded the HIP runtime: errors are ignored)
  if (hi_) (void)hipFree(hi_);
  if (slot_) (void)hipFree(slot_);
}
bool PlaneSet::ReserveParts() {
  if (!slot_) {
    void *p = nullptr;
    if (hipMalloc(&p, 256 + sizeof(float) * kS16MaxParts) != hipSuccess) { set_error("PlaneSet: hipMalloc failed"); return false; }
    slot_ = static_cast<unsigned *>(p);
    parts_ = reinterpret_cast<float *>(static_cast<char *>(p) + 256);
    (void)hipMemsetAsync(p, 0, 256 + sizeof(float) * kS16MaxParts, cur_stream());
    host_bound_ = -1.f;
  }
  return true;
}
bool PlaneSet::Reserve(int rows, int cols) {
  if (rows <= 0 || cols <= 0) return false;
  const int ld = s16_plane_ld(cols), rows_p = (rows + kS16Pad - 1) / kS16Pad * kS16Pad;
  const size_t need = (size_t)rows_p * ld;
  if (!ReserveParts()) return false;
  const bool reshape = rows != rows_ || cols != cols_;
  if (need > cap_) {
    if (hi_) {
      (void)hipStreamSynchronize(cur_stream());   // outstanding products may still read the old planes
      (void)hipFree(hi_);
      hi_ = lo_ = nullptr;
      cap_ = 0;
    }
    void *p = nullptr;
    if (hipMalloc(&p, 2 * need * sizeof(h16)) != hipSuccess) { set_error("PlaneSet: hipMalloc failed"); return false; }
    hi_ = static_cast<h16 *>(p);
    cap_ = need;
  }
  if (reshape) {
    lo_ = hi_ + need;
    rows_ = rows; cols_ = cols; ld_ = ld; rows_p_ = rows_p;
    (void)hipMemsetAsync(hi_, 0, 2 * need * sizeof(h16), cur_stream());   // the padding stays zero from here on
    Invalidate();
  }
  return true;
}
bool PlaneSet::SetBound(float bound) {
  if (!slot_) return false;
  if (bound != host_bound_) {
    (void)hipMemcpyAsync(slot_, &bound, sizeof(float), hipMemcpyHostToDevice, cur_stream());   // (pageable source: copied before the call returns)
    host_bound_ = bound;
  }
  return true;
}
// a width the conversions take: a multiple of 4, or any under gemm_split16_ragged() (the base and the stride stay 16-byte aligned)
static bool s16_width_ok(int cols) { return !(cols & 3) || gemm_split16_ragged(); }
bool PlaneSet::ConvertWithParts(const float *src, int rows, int cols, int stride, int nparts) {
  if (!s16_width_ok(cols) || (stride & 3) || !aligned16(src) || nparts > kS16MaxParts) return false;
  if (!Reserve(rows, cols)) return false;
  host_bound_ = -1.f;
  ConvJobs js;
  js.j[0] = ConvJob{src, stride, View(), parts_, nparts};
  launch_convert(js, 1, std::min(rows_p_, 512));
  return true;
}
bool PlaneSet::ConvertFrom(const float *src, int rows, int cols, int stride) {
  if (!s16_width_ok(cols) || (stride & 3) || !aligned16(src)) return false;
  if (!Reserve(rows, cols)) return false;
  {
    const CoopConvJob job = {src, stride, nullptr, 0, View(), nullptr, 0};
    if (coop_convert_launch(&job, 1)) { host_bound_ = -1.f; return true; }   // one launch instead of two
  }
  MaxJobs ms;
  ms.j[0] = MaxJob{src, rows, cols, stride, parts_};
  launch_absmax(ms, 1);
  return ConvertWithParts(src, rows, cols, stride, kS16ConvParts);
}
// several matrices in one maximum launch and one conversion launch (the recurrent layers convert up to seven small tensors at a time)
bool PlaneSet::ConvertMany(const ConvertSpec *specs, int n, const SeqFillJob *fill, bool *fill_done) {
  if (fill_done) *fill_done = false;
  if (n <= 0 || n > kS16MaxJobs) return false;
  MaxJobs ms;
  ConvJobs js;
  int max_rows = 0;
  bool need_max = false;
  for (int i = 0; i < n; i++) {
    const ConvertSpec &c = specs[i];
    if (!c.planes || !c.src || !s16_width_ok(c.cols) || (c.stride & 3) || !aligned16(c.src)) return false;
    if (!c.planes->Reserve(c.rows, c.cols)) return false;
    c.planes->host_bound_ = -1.f;
    const bool given = c.parts != nullptr && c.nparts > 0 && c.nparts <= kS16MaxParts;
    need_max = need_max || !given;
    ms.j[i] = MaxJob{c.src, c.rows, c.cols, c.stride, c.planes->parts_};
    js.j[i] = given ? ConvJob{c.src, c.stride, c.planes->View(), c.parts, c.nparts} : ConvJob{c.src, c.stride, c.planes->View(), c.planes->parts_, kS16ConvParts};
    max_rows = std::max(max_rows, c.planes->rows_p_);
  }
  if (need_max) {   // one launch for the maxima and the planes where the matrices fit one resident grid
    CoopConvJob cj[kS16MaxJobs];
    for (int i = 0; i < n; i++) {
      const ConvertSpec &c = specs[i];
      const bool given = c.parts != nullptr && c.nparts > 0 && c.nparts <= kS16MaxParts;
      cj[i] = CoopConvJob{c.src, c.stride, nullptr, 0, c.planes->View(), given ? c.parts : nullptr, given ? c.nparts : 0};
    }
    if (coop_convert_launch(cj, n, fill)) {
      if (fill_done) *fill_done = fill != nullptr;
      return true;
    }
  }
  if (need_max) launch_absmax(ms, n);
  launch_convert(js, n, std::min(max_rows, 512));
  return true;
}
const float *PlaneSet::OneBound() {
  static float *one = [] {
    float *p = nullptr;
    const float v = 1.0f;
    if (hipMalloc(&p, 256) != hipSuccess || hipMemcpy(p, &v, sizeof(v), hipMemcpyHostToDevice) != hipSuccess) { set_error("PlaneSet::OneBound: allocation failed"); return static_cast<float *>(nullptr); }
    return p;
  }();
  return one;
}

// C = epilogue(alpha op(A) op(B) + beta C) from planes.  a_kc: A is stored [M x K] (else [K x M]); b_kc: B is stored [N x K]
// (else [K x N]).  For a pair (g.pair) a1 / b1 are the second product's operands.  false: not eligible (nothing was launched).
// Column statistics and (transposed A) column sums are formed in the kernel.
bool gemm_split16_planes_launch(GemmArgs &g, bool a_kc, bool b_kc, const S16View &a, const S16View &b, const S16View *a1, const S16View *b1,
                                int cfg) {
  if (g.split_k > 1) return false;   // (the split is chosen here, not by the caller)
  if (g.M < 64 || g.N < 64 || g.K < 32) return false;
  if (g.pair && (!a1 || !b1)) return false;
  S16Operands ops;
  ops.a = a; ops.b = b;
  ops.a1 = a1 ? *a1 : a; ops.b1 = b1 ? *b1 : b;
  ops.kp = (g.K + BKH - 1) / BKH * BKH;
  // the planes must describe the operands of this product
  auto fits = [&](const S16View &v, bool kc, int outer) { return v.hi && (kc ? (v.rows == outer && v.cols == g.K) : (v.rows == g.K && v.cols == outer)); };
  if (!fits(ops.a, a_kc, g.M) || !fits(ops.b, b_kc, g.N) || !fits(ops.a1, a_kc, g.M) || !fits(ops.b1, b_kc, g.N)) return false;
  t_last_parts = 0;
  const int planes = gemm_operand_planes();
  auto asks = [&](const aslp_gemm_epilogue &ep, float *C) {
    GemmArgs g1 = g;
    g1.C = C; g1.ep = ep;
    S16Asks s;
    s.planes_of = ep.planes_of; s.wmax = ep.wmax_parts != nullptr; s.cmax = ep.cmax_parts != nullptr;
    s.amax = ep.amax_parts != nullptr && ep.act_out != nullptr;
    s.colstats = ep.colstats != nullptr; s.colsum = ep.colsum != nullptr;
    s.wide_ok = g.wide_epilogue && gemm_epilogue_wide_ok(g1);
    return s;
  };
  S16Plan p = s16_plan(g.M, g.N, g.K, a_kc, b_kc, g.pair != 0, asks(g.ep, g.C), g.pair ? asks(g.ep1, g.C1) : S16Asks(), planes, cfg, s16_tuning());
  auto drop_extras = [](aslp_gemm_epilogue &ep) { ep.planes_of = 0; ep.wmax_parts = ep.cmax_parts = ep.amax_parts = nullptr; ep.bound_w_parts = ep.bound_c_parts = nullptr; };
  auto drop_maxima = [](aslp_gemm_epilogue &ep) {
    if (ep.planes_of == 1) { ep.planes_of = 0; ep.bound_w_parts = ep.bound_c_parts = nullptr; }
    ep.wmax_parts = ep.cmax_parts = ep.amax_parts = nullptr;
  };
  if (g.ep.act_out == nullptr) g.ep.amax_parts = nullptr;   // (maxima of an output that is not written)
  if (g.ep1.act_out == nullptr) g.ep1.amax_parts = nullptr;
  if (p.drop_extras) drop_extras(g.ep);
  if (p.drop_extras1) drop_extras(g.ep1);
  if (p.drop_maxima) { drop_maxima(g.ep); if (g.pair) drop_maxima(g.ep1); }
  auto launch = [&](GemmArgs &ga, int tile) {
    const bool extra = ga.ep.planes_of != 0 || ga.ep.wmax_parts != nullptr || ga.ep.cmax_parts != nullptr || ga.ep.amax_parts != nullptr ||
                       (ga.pair && (ga.ep1.planes_of != 0 || ga.ep1.wmax_parts || ga.ep1.cmax_parts || ga.ep1.amax_parts));
    if (a_kc && b_kc) s16_launch_tile<true, true>(ga, ops, tile, extra);
    else if (a_kc && !b_kc) s16_launch_tile<true, false>(ga, ops, tile, extra);
    else if (!a_kc && !b_kc) s16_launch_tile<false, false>(ga, ops, tile, extra);
    else s16_launch_tile<false, true>(ga, ops, tile, extra);
    t_last_cfg_s16 = tile;
  };
  if (p.split_k >= 2) {
    const long stride = (long)g.M * g.N;
    const int np = g.pair ? 2 : 1;
    float *part = static_cast<float *>(scratch(kScratchSplitK, sizeof(float) * (size_t)stride * p.split_k * np));
    if (part) {
      GemmArgs pg = g;
      pg.C = part; pg.ldc = g.N; pg.alpha = 1.0f; pg.beta = 0.0f; pg.ep = aslp_gemm_epilogue();
      pg.C1 = part + (size_t)stride * p.split_k; pg.ep1 = aslp_gemm_epilogue();
      pg.split_k = p.split_k; pg.k_chunk = p.k_chunk; pg.split_stride = stride;
      launch(pg, p.tile);
      GemmArgs r = g;
      r.split_k = 0;
      const int wgs = gemm_splitk_reduce(part, p.split_k, stride, r);
      t_last_parts = (r.ep.planes_of == 2 || r.ep.cmax_parts || r.ep.amax_parts) ? wgs : 0;
      return true;
    }
    S16Tuning whole = s16_tuning();   // no scratch for the chunks: the product in one launch
    whole.splitk = 0;
    p = s16_plan(g.M, g.N, g.K, a_kc, b_kc, g.pair != 0, asks(g.ep, g.C), g.pair ? asks(g.ep1, g.C1) : S16Asks(), planes, cfg, whole);
  }
  if (p.tile == 0) return false;
  launch(g, p.tile);
  return true;
}


// The same with either operand given as fp32 only (pa / pb NULL): its planes are made in the call's scratch, by a maximum pass and a
// conversion in front of the product.
bool gemm_split16_launch(GemmArgs &g, bool a_kc, bool b_kc, int cfg, const S16View *pa, const S16View *pb) {
  if (g.pair || g.split_k > 1) return false;
  if (g_split16_tile_override >= 0) cfg = g_split16_tile_override;
  if (!gemm_split16_serves(g.M, g.N, g.K)) return false;
  if ((!pa && !(g.A && g.a_vec)) || (!pb && !(g.B && g.b_vec))) return false;
  if (pa && pb) return gemm_split16_planes_launch(g, a_kc, b_kc, *pa, *pb, nullptr, nullptr, cfg);
  auto pad = [](int x) { return (x + kS16Pad - 1) / kS16Pad * kS16Pad; };
  const int a_rows = a_kc ? g.M : g.K, a_cols = a_kc ? g.K : g.M, b_rows = b_kc ? g.N : g.K, b_cols = b_kc ? g.K : g.N;
  const size_t plane_a = pa ? 0 : (size_t)pad(a_rows) * s16_plane_ld(a_cols), plane_b = pb ? 0 : (size_t)pad(b_rows) * s16_plane_ld(b_cols);
  const size_t head = 256 + sizeof(float) * 2 * kS16ConvParts;
  const size_t bytes = head + sizeof(h16) * 2 * (plane_a + plane_b);
  unsigned char *buf = static_cast<unsigned char *>(scratch(kScratchSplit16, bytes));
  if (!buf) return false;
  unsigned *slots = reinterpret_cast<unsigned *>(buf);
  float *part = reinterpret_cast<float *>(buf + 256);
  h16 *ah = reinterpret_cast<h16 *>(buf + head), *al = ah + plane_a, *bh = al + plane_a, *bl = bh + plane_b;
  const S16View va = pa ? *pa : S16View{ah, al, s16_plane_ld(a_cols), a_rows, a_cols, slots};
  const S16View vb = pb ? *pb : S16View{bh, bl, s16_plane_ld(b_cols), b_rows, b_cols, slots + 1};
  const MaxJob ma = {g.A, a_rows, a_cols, g.lda, part}, mb = {g.B, b_rows, b_cols, g.ldb, part + kS16ConvParts};
  const ConvJob ca = {g.A, g.lda, va, part, kS16ConvParts}, cb = {g.B, g.ldb, vb, part + kS16ConvParts, kS16ConvParts};
  // One launch for maxima and planes where the matrices fit one resident grid (nn_fused.hip copy_planes_coop) -- which writes the matrix
  // region only: scratch planes are not zeroed, so only for operands without padding rows / columns.
  {
    auto unpadded = [&](const S16View &v) { return pad(v.rows) == v.rows && v.ld == v.cols; };
    CoopConvJob cj[2];
    int n = 0;
    bool ok = true;
    if (!pa) { cj[n++] = CoopConvJob{g.A, g.lda, nullptr, 0, va, nullptr, 0}; ok = ok && unpadded(va); }
    if (!pb) { cj[n++] = CoopConvJob{g.B, g.ldb, nullptr, 0, vb, nullptr, 0}; ok = ok && unpadded(vb); }
    if (ok && n > 0 && coop_convert_launch(cj, n)) return gemm_split16_planes_launch(g, a_kc, b_kc, va, vb, nullptr, nullptr, cfg);
  }
  // (matrices in one launch share the threads-per-row choice: the widest one's)
  MaxJobs ms;
  ConvJobs js;
  if (!pa && !pb) {
    ms.j[0] = ma; ms.j[1] = mb; js.j[0] = ca; js.j[1] = cb;
    launch_absmax(ms, 2);
    launch_convert(js, 2, 512);
  } else {
    ms.j[0] = pa ? mb : ma;
    js.j[0] = pa ? cb : ca;
    launch_absmax(ms, 1);
    launch_convert(js, 1, 512);
  }
  return gemm_split16_planes_launch(g, a_kc, b_kc, va, vb, nullptr, nullptr, cfg);
}

int gemm_split16_last_parts() { return t_last_parts; }
int gemm_split16_last_tile() { return t_last_cfg_s16; }
void gemm_split16_reset_last_parts() { t_last_parts = 0; }
// most per-workgroup maxima a split-fp16 product of this output shape leaves (the caller's arrays must hold them)
int gemm_split16_max_parts(int M, int N) { return std::max(((M + 63) / 64) * ((N + 127) / 128), ((M + 31) / 32) * ((N + 63) / 64) <= 256 ? ((M + 31) / 32) * ((N + 63) / 64) : 0); }

}  // namespace aslp
extern "C" {
int aslp_gemm_split16_plan(int transA, int transB, int M, int N, int K, int ldc, const aslp_gemm_epilogue *ep, const aslp_gemm_epilogue *ep1,
                           int planes, int cfg, int *split_k) {
  using namespace aslp;
  if (split_k) *split_k = 0;
  if (!gemm_split16_serves(M, N, K)) return 0;
  auto asks = [&](const aslp_gemm_epilogue *e) {
    S16Asks s;
    GemmArgs g = {};
    g.N = N; g.ldc = ldc;
    if (e) {
      g.ep = *e;
      s.planes_of = e->planes_of; s.wmax = e->wmax_parts != nullptr; s.cmax = e->cmax_parts != nullptr;
      s.amax = e->amax_parts != nullptr && e->act_out != nullptr;
      s.colstats = e->colstats != nullptr; s.colsum = e->colsum != nullptr;
    }
    s.wide_ok = gemm_epilogue_wide_ok(g);
    return s;
  };
  const S16Plan p = s16_plan(M, N, K, !transA, transB != 0, ep1 != nullptr, asks(ep), asks(ep1), (planes == 1 || planes == 2) ? planes : gemm_operand_planes(), cfg,
                             s16_tuning());
  if (split_k) *split_k = p.split_k;
  return p.tile;
}
void aslp_keep_weight_planes(int on) { aslp::g_keep_override = on < 0 ? -1 : (on != 0); }
void aslp_params_changed(void) {
  aslp::join_side_stream();   // weight updates the calling thread's latest backward pass left running beside it (Nnet::Backpropagate): the caller is about to touch the parameters
  aslp::g_param_epoch.fetch_add(1, std::memory_order_relaxed);
}
void aslp_gemm_split16(int on) { aslp::g_split16_override = on < 0 ? -1 : (on != 0); }
void aslp_gemm_split16_tile(int cfg) { aslp::g_split16_tile_override = cfg < 0 ? -1 : cfg; }
void aslp_gemm_operand_planes(int n) { aslp::g_operand_planes_override = (n == 1 || n == 2) ? n : -1; }
int aslp_gemm_operand_planes_get(void) { return aslp::gemm_operand_planes(); }
void aslp_gemm_split16_ragged(int on) { aslp::g_ragged_override = on < 0 ? -1 : (on != 0); }
int aslp_gemm_split16_ragged_get(void) { return aslp::gemm_split16_ragged() ? 1 : 0; }
int aslp_gemm_last_parts(void) { return aslp::gemm_split16_last_parts(); }
void aslp_weight_bound(const float *w_parts, int n_w, const float *c_parts, int n_c, const aslp_planes *a, const aslp_planes *b, int K, float alpha,
                       float beta, float w_alpha, float clip, aslp_planes *w_planes) {
  using namespace aslp;
  if (!w_parts || n_w <= 0 || !a || !b || !w_planes) { set_error("aslp_weight_bound: missing argument"); return; }
  BoundJob j = {w_parts, n_w, c_parts, c_parts ? n_c : 0, reinterpret_cast<const PlaneSet *>(a)->Slot(), reinterpret_cast<const PlaneSet *>(b)->Slot(),
                (float)K, alpha, beta, w_alpha, clip, reinterpret_cast<PlaneSet *>(w_planes)->Slot()};
  hipLaunchKernelGGL(s16_weight_bound_kernel, dim3(1), dim3(256), 0, cur_stream(), j);
  reinterpret_cast<PlaneSet *>(w_planes)->ForgetHostBound();
  check_launch("aslp_weight_bound");
}
void aslp_absmax_parts(const float *src, MatrixDim d, float *parts) {
  using namespace aslp;
  if (!src || !parts || !s16_width_ok(d.cols) || (d.stride & 3) || !aligned16(src)) { set_error("aslp_absmax_parts: unsupported matrix"); return; }
  MaxJobs ms;
  ms.j[0] = MaxJob{src, d.rows, d.cols, d.stride, parts};
  launch_absmax(ms, 1);
  check_launch("aslp_absmax_parts");
}
}
