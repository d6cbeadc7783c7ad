// rnn_fused.hip -- one launch per timestep for the LSTM recurrence (both directions at once).
//
// The reference runs, per timestep and direction, a skinny cuBLAS GEMM (S x 4C x R), ~18 elementwise
// launches and a second skinny GEMM (S x R x C) (nnet-blstm-projected-streams-lc.h:571-609); with
// M = S = 32 streams those GEMMs use a handful of CUs and are pure latency.  Here the recurrence is
// re-associated so that only ONE product sits on the sequential path:
//     gates(t) = [x(t) W_x^T + b]  +  m(t-1) W_eff^T,      W_eff = W_r W_rm   (4C x C;  = W_r without projection)
// and the projection r = m W_rm^T is taken out of the loop (one batched GEMM over all t).  The step
// kernel fuses that product with the whole gate block: a workgroup owns 8 cells x 32 streams, i.e. a
// 32 x 32 MFMA tile whose columns are the (g,i,f,o) pre-activations of its 8 cells; its 4 waves split
// K = C, operands go global -> VGPR as 16-B loads (both are K-contiguous, no LDS staging), partial
// tiles are summed through LDS in wave order (deterministic) and the 256 threads then each finish one
// (stream, cell): peepholes, sigmoid/tanh, cell clip, c/h/m -- one launch, C/8 x S/32 x ndir workgroups.
// W_eff's row slices are pinned to a workgroup index, hence to one XCD's L2, across the T launches.
// Backward mirrors it:  d_m(t) = dm_ext(t) + dGATES(t+1) W_eff  (K = 4C, split over 4 workgroups x 4 waves,
// partials to scratch) followed by the fused gate-block backward, which adds the partials in a fixed order.
// Opt-in (aslp_lstm_step_split16): the same two products on v_mfma_f32_32x32x16_f16 with operands as fp16 pieces (lstm_step_fwd_h,
// lstm_step_bwd_gemm_h; contract in include/aslp_kernels.h).  A kernel and its _h counterpart differ in the product alone: the forward
// pair shares its prologue and gate block (step_fwd_cell_load / step_fwd_cell_finish), the backward pair its reduction
// (step_bwd_store_partial).  The fp32-instruction kernels call product_f32 of rnn_mfma.h; the _h kernels hold product_h / product_t_h
// inline, for the reason given above lstm_step_fwd_h.
#include "aslp_kernels.h"
#include "common.h"
#include "scratch.h"
#include "rnn_mfma.h"

namespace aslp {
namespace {

constexpr int kCB = 8;    // cells per forward workgroup (x 4 gates = 32 MFMA columns)
constexpr int kKQ = 8;    // K-split of the backward product across workgroups (one round of 8 loads per wave at C = 512; 4: 7.85, 8: 7.42, 16: 8.17 ms per LC step)
constexpr int kFwdU = 8;   // K-chunks in flight in the forward product (16: 7.60 vs 7.45 ms per LC step)
constexpr int kNW = 4;    // waves per step workgroup (K split 4 ways; 8 waves were measured slower: 8.15 vs 7.85 ms on the LC step)

// One thread's (stream, cell) of a forward step: its epilogue operands, requested before the product so their latency hides under it ...
// lstm_step_fwd and lstm_step_fwd_h share this and the gate block below.  Built from them lstm_step_fwd<false> takes 32 instead of 34
// SGPRs and both lstm_step_fwd one instruction more; the forward recurrence measured inside the range of the commit before at both of
// the recipes' shapes (profiles/step_kernels_shared_text.txt).
template <bool CIFG>
struct StepFwdCell {
  float *ys;
  int sl, cc, c;
  bool live, masked;
  float xg, xf, xo, xi, cprev, pf, po, pi;
};
template <bool CIFG>
__device__ __forceinline__ StepFwdCell<CIFG> step_fwd_cell_load(const aslp_lstm_step_dir &D, int C, int S, int ld, int s0, int c0) {
  constexpr int G = CIFG ? 3 : 4;
  constexpr int gi = 1, gf = CIFG ? 1 : 2, go = CIFG ? 2 : 3;
  const int oc = G * C;
  StepFwdCell<CIFG> e;
  e.sl = threadIdx.x / kCB; e.cc = threadIdx.x % kCB;
  const int s = s0 + e.sl;
  e.c = c0 + e.cc;
  e.live = threadIdx.x < 256 && s < S && e.c < C;  // the first 4 waves finish the 256 (stream, cell) pairs
  e.ys = D.y_cur + (long)(e.live ? s : 0) * ld;
  const int cq = e.live ? e.c : 0;
  e.xg = e.ys[cq]; e.xf = e.ys[gf * C + cq]; e.xo = e.ys[go * C + cq]; e.xi = CIFG ? 0.f : e.ys[gi * C + cq];
  e.cprev = D.y_prev[(long)(e.live ? s : 0) * ld + oc + cq];
  e.pf = D.peep_f[cq]; e.po = D.peep_o[cq]; e.pi = CIFG ? 0.f : D.peep_i[cq];
  e.masked = D.seq_lengths && D.t > D.seq_lengths[e.live ? s : 0];
  return e;
}
// ... and the gate block on the 4 waves' partial tiles, added in wave order (call after the barrier)
template <bool CIFG>
__device__ __forceinline__ void step_fwd_cell_finish(const StepFwdCell<CIFG> &e, const float (*red)[32 * kPad], int C) {
  constexpr int G = CIFG ? 3 : 4;
  constexpr int gi = 1, gf = CIFG ? 1 : 2, go = CIFG ? 2 : 3;
  const int GC = G * C, oc = GC, oh = GC + C, om = GC + 2 * C;
  if (!e.live) return;
  float *ys = e.ys;
  const int c = e.c;
  float pre[G];
#pragma unroll
  for (int g = 0; g < G; g++) pre[g] = tile_sum<kNW>(red, e.sl, g * kCB + e.cc);
  if (e.masked) {  // nnet-blstm-projected-streams.h:654-657
    ys[c] = 0.f; ys[gf * C + c] = 0.f; ys[go * C + c] = 0.f; ys[oc + c] = 0.f; ys[oh + c] = 0.f; ys[om + c] = 0.f;
    if (!CIFG) ys[gi * C + c] = 0.f;
    return;
  }
  const float g = tanh_ref(e.xg + pre[0]);
  const float f = sigmoid_ref(e.xf + pre[gf] + e.cprev * e.pf);
  float cell;
  if (!CIFG) {
    const float i = sigmoid_ref(e.xi + pre[gi] + e.cprev * e.pi);
    ys[gi * C + c] = i;
    cell = g * i + e.cprev * f;
  } else {
    cell = -g * f + g + e.cprev * f;
  }
  cell = fminf(fmaxf(cell, -50.0f), 50.0f);
  const float hh = tanh_ref(cell);
  const float o = sigmoid_ref(e.xo + pre[go] + cell * e.po);
  ys[c] = g; ys[gf * C + c] = f; ys[go * C + c] = o; ys[oc + c] = cell; ys[oh + c] = hh; ys[om + c] = hh * o;
}

// One forward step.  Rows of invalid (gate, cell) / stream pairs read row 0 / the last stream and their outputs are not stored.
template <bool CIFG>
__global__ void __launch_bounds__(64 * kNW) lstm_step_fwd(aslp_lstm_step a) {
  __shared__ float red[kNW][32 * kPad];
  constexpr int G = CIFG ? 3 : 4;
  const aslp_lstm_step_dir D = a.dir[blockIdx.z];
  const int C = a.C, S = a.S, ld = a.ld;
  const int om = G * C + 2 * C;
  const int c0 = blockIdx.x * kCB, s0 = blockIdx.y * 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31;
  const StepFwdCell<CIFG> e = step_fwd_cell_load<CIFG>(D, C, S, ld, s0, c0);
  const int gate = l31 / kCB, cell = c0 + (l31 % kCB);
  const bool nvalid = gate < G && cell < C;
  const float *arow = D.y_prev + (long)min(s0 + l31, S - 1) * ld + om;       // m(t-1) of this lane's stream
  const float *brow = D.w + (long)(nvalid ? gate * C + cell : 0) * a.ldw;    // W_eff row of (gate, cell)
  product_f32<kFwdU>(red[wave], arow, brow, C, wave, kNW, lane, !D.no_product);
  __syncthreads();
  step_fwd_cell_finish<CIFG>(e, red, C);
}

// The same step with the product on v_mfma_f32_32x32x16_f16 (aslp_lstm_step_split16): m(t-1) split into NP fp16 pieces as it is loaded
// (|m| <= 1: no scale), W_eff from its planes (ah.w_hi / w_lo, scaled by the bound in *ah.w_slot); same grid, same K split over the 4
// waves (contiguous runs of 16-wide k steps), same reduction and gate block.
// The product is product_h of rnn_mfma.h, kept here statement for statement: called as that function the four kernels came out of the
// compiler with other text (2 to 4 instructions more, up to 10 SGPRs fewer) and the forward recurrence measured 0.3 % to 1.8 % FASTER than
// the commit before, below its window-to-window range in every case (profiles/step_kernels_shared_text.txt), which is not what a change
// that sets out to move nothing may bring along.  Calling product_h here is that speed-up, to be taken on its own.
template <bool CIFG, int NP>
__global__ void __launch_bounds__(64 * kNW) lstm_step_fwd_h(aslp_lstm_step_h ah) {
  __shared__ float red[kNW][32 * kPad];
  constexpr int G = CIFG ? 3 : 4;
  const aslp_lstm_step_dir D = ah.step.dir[blockIdx.z];
  const int C = ah.step.C, S = ah.step.S, ld = ah.step.ld;
  const int om = G * C + 2 * C;
  const int c0 = blockIdx.x * kCB, s0 = blockIdx.y * 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31;
  const StepFwdCell<CIFG> e = step_fwd_cell_load<CIFG>(D, C, S, ld, s0, c0);
  const int gate = l31 / kCB, cell = c0 + (l31 % kCB);
  const bool nvalid = gate < G && cell < C;
  const float *arow = D.y_prev + (long)min(s0 + l31, S - 1) * ld + om;
  const long boff = (long)(nvalid ? gate * C + cell : 0) * ah.ldp;
  const h16 *bhi = static_cast<const h16 *>(ah.w_hi[blockIdx.z]) + boff;
  const h16 *blo = NP == 2 ? static_cast<const h16 *>(ah.w_lo[blockIdx.z]) + boff : bhi;
  {
    const int h = lane >> 5;
    const float inv_w = ldexpf(1.0f, -s16_exponent(*ah.w_slot[blockIdx.z]));
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, acx = acc;
    const int nst = (C + 15) / 16, per = (nst + kNW - 1) / kNW, qend = min(nst, (wave + 1) * per);
    if (!D.no_product)
      for (int q0 = wave * per; q0 < qend; q0 += kRunH) mfma_run_h<NP, kRunH, false, false>(acc, acx, arow, C, bhi, blo, q0, qend, h, nullptr);
    if (NP == 2) acc += acx * (1.0f / 2048.f);
    acc *= inv_w;
    store_tile(red[wave], acc, lane);
  }
  __syncthreads();
  step_fwd_cell_finish<CIFG>(e, red, C);
}

// the 4 waves' partial tiles, added in wave order, to partial[slab][s][c] (slab = direction x K-part)
__device__ __forceinline__ void step_bwd_store_partial(const float (*red)[32 * kPad], float *__restrict__ partial, long slab, int S, int C, int s0, int c0) {
  float *out = partial + (slab * S) * C;
  for (int e = threadIdx.x; e < 32 * 32; e += 64 * kNW) {
    const int sl = e >> 5, n = e & 31;
    if (s0 + sl < S && c0 + n < C) out[(long)(s0 + sl) * C + c0 + n] = tile_sum<kNW>(red, sl, n);
  }
}

// partial[dir][kq][s][c] = sum over this workgroup's K-part of dGATES(next)[s][k] * W_eff^T[c][k]; the K slice is part kq * kNW + wave of
// kNW * kKQ
template <int G>
__global__ void __launch_bounds__(64 * kNW) lstm_step_bwd_gemm(aslp_lstm_step a, float *__restrict__ partial) {
  __shared__ float red[kNW][32 * kPad];
  const aslp_lstm_step_dir D = a.dir[blockIdx.z];
  const int C = a.C, S = a.S, ld = a.ld, GC = G * C;
  const int c0 = blockIdx.x * 32, kq = blockIdx.y % kKQ, s0 = (blockIdx.y / kKQ) * 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31;
  const float *arow = D.d_next + (long)min(s0 + l31, S - 1) * ld;          // dGATES(next), columns [0, GC)
  const float *brow = D.w + (long)min(c0 + l31, C - 1) * a.ldw;            // W_eff^T row of cell c0 + l31
  product_f32(red[wave], arow, brow, GC, kq * kNW + wave, kNW * kKQ, lane, true);
  __syncthreads();
  step_bwd_store_partial(red, partial, blockIdx.z * kKQ + kq, S, C, s0, c0);
}

// The same partial products on v_mfma_f32_32x32x16_f16 (aslp_lstm_step_split16), taken transposed: dGATES sits behind a power-of-two
// scale per stream row and run of kRunH k steps (128 consecutive k; one wave's K slice for C <= 1024).  Same grid, K split and reduction
// as lstm_step_bwd_gemm.  The product is product_t_h of rnn_mfma.h, kept here statement for statement for the reason given above
// lstm_step_fwd_h (as a call: 1 to 13 instructions more, 4 VGPRs fewer with two pieces, the backward recurrence 0.5 % to 1.4 % faster, below the range in
// three of four cases).
template <int G, int NP>
__global__ void __launch_bounds__(64 * kNW) lstm_step_bwd_gemm_h(aslp_lstm_step_h ah, float *__restrict__ partial) {
  __shared__ float red[kNW][32 * kPad];
  const aslp_lstm_step_dir D = ah.step.dir[blockIdx.z];
  const int C = ah.step.C, S = ah.step.S, ld = ah.step.ld, GC = G * C;
  const int c0 = blockIdx.x * 32, kq = blockIdx.y % kKQ, s0 = (blockIdx.y / kKQ) * 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31;
  const float *drow = D.d_next + (long)min(s0 + l31, S - 1) * ld;          // dGATES(next), columns [0, GC)
  const long woff = (long)min(c0 + l31, C - 1) * ah.ldp;                  // W_eff^T row of cell c0 + l31
  const h16 *whi = static_cast<const h16 *>(ah.w_hi[blockIdx.z]) + woff;
  const h16 *wlo = NP == 2 ? static_cast<const h16 *>(ah.w_lo[blockIdx.z]) + woff : whi;
  {
    const int h = lane >> 5;
    const float inv_w = ldexpf(1.0f, -s16_exponent(*ah.w_slot[blockIdx.z]));
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x16 tot = zero;
    const int nst = (GC + 15) / 16, per = (nst + kNW * kKQ - 1) / (kNW * kKQ), part = kq * kNW + wave, qend = min(nst, (part + 1) * per);
    for (int q0 = part * per; q0 < qend; q0 += kRunH) {
      f32x16 acc = zero, acx = zero;
      float inv_s = 1.0f;
      mfma_run_h<NP, kRunH, true, true>(acc, acx, drow, GC, whi, wlo, q0, qend, h, &inv_s);
      if (NP == 2) acc += acx * (1.0f / 2048.f);
      tot += acc * inv_s;
    }
    tot *= inv_w;
    store_tile_t(red[wave], tot, lane);
  }
  __syncthreads();
  step_bwd_store_partial(red, partial, (int)(blockIdx.z * kKQ + kq), S, C, s0, c0);   // (int): the slab index sign-extended, as this kernel always had it
}

// gate-block backward of step t for every direction; d_m = dm_ext (already in the m column) + the K-split partials
template <bool CIFG>
__global__ void __launch_bounds__(kBlock) lstm_step_bwd_cell(aslp_lstm_step a, const float *__restrict__ partial, int with_partial) {
  constexpr int G = CIFG ? 3 : 4;
  const aslp_lstm_step_dir D = a.dir[blockIdx.y];
  const int C = a.C, S = a.S, ld = a.ld;
  const int GC = G * C, oc = GC, oh = GC + C, om = GC + 2 * C;
  const int og = 0, oi = C, of = CIFG ? C : 2 * C, oo = CIFG ? 2 * C : 3 * C;
  const int n = S * C;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += gridDim.x * blockDim.x) {
    const int s = idx / C, c = idx - s * C;
    const long o_ = (long)s * ld;
    // every load of this (stream, cell) first, stores last: the compiler cannot move a load above a store through a pointer
    // that might alias it, and a store in the middle would split the loads into two dependent rounds of memory latency
    float dm = D.d_cur[o_ + om + c];
    float psum[kKQ];
    if (with_partial) {
      const float *p = partial + ((long)blockIdx.y * kKQ * S + s) * C + c;
#pragma unroll
      for (int q = 0; q < kKQ; q++) psum[q] = p[(long)q * S * C];
    }
    const float yo = D.y_cur[o_ + oo + c], yh = D.y_cur[o_ + oh + c], yg = D.y_cur[o_ + og + c], yf = D.y_cur[o_ + of + c];
    const float yi = CIFG ? 0.f : D.y_cur[o_ + oi + c];
    const float dn_c = D.d_next[o_ + oc + c], yn_f = D.y_next[o_ + of + c], dn_f = D.d_next[o_ + of + c];
    const float dn_i = CIFG ? 0.f : D.d_next[o_ + oi + c];
    const float pi = CIFG ? 0.f : D.peep_i[c], pf = D.peep_f[c], po = D.peep_o[c];
    const float cprev = D.y_prev[o_ + oc + c];
    if (with_partial) {
#pragma unroll
      for (int q = 0; q < kKQ; q++) dm += psum[q];
      D.d_cur[o_ + om + c] = dm;  // the reference's d_m (lc.h:793) -- kept for InfoGradient-style dumps
    }
    const float dh = dtanh(yh, dm * yo);
    const float dov = dsigm(yo, dm * yh);
    float dc = dh + dn_c * yn_f;
    if (!CIFG) dc += dn_i * pi;
    dc += dn_f * pf;
    dc += dov * po;
    D.d_cur[o_ + oh + c] = dh;
    D.d_cur[o_ + oo + c] = dov;
    D.d_cur[o_ + oc + c] = dc;
    if (!CIFG) {
      D.d_cur[o_ + of + c] = dsigm(yf, dc * cprev);
      D.d_cur[o_ + oi + c] = dsigm(yi, dc * yg);
      D.d_cur[o_ + og + c] = dtanh(yg, dc * yi);
    } else {
      D.d_cur[o_ + of + c] = dsigm(yf, dc * cprev - dc * yg);
      D.d_cur[o_ + og + c] = dtanh(yg, dc - dc * yf);
    }
  }
}

bool step_args_ok(const aslp_lstm_step *a, const char *who) {
  if (!a || a->ndir < 1 || a->ndir > 2 || a->S <= 0 || a->C <= 0 || (a->C & 3) || (a->ld & 3) || (a->ldw & 3)) {
    set_error(std::string(who) + ": bad arguments (needs 1..2 directions, C, ld, ldw multiples of 4)");
    return false;
  }
  return true;
}

// the planes a split-fp16 step launch reads (K = C forward, G C backward), per direction
bool step_planes_ok(const aslp_lstm_step_h *a, int K, int np, const char *who) {
  bool ok = true;
  for (int d = 0; ok && d < a->step.ndir; d++) ok = planes_ok(a->w_hi[d], a->w_lo[d], a->w_slot[d], a->ldp, K, np);
  if (!ok) set_error(std::string(who) + ": bad planes (needs hi / lo / slot per direction, 16-byte aligned, ldp a multiple of 8 and >= K rounded up to 16)");
  return ok;
}

// split-fp16 products on this path: opt-in (aslp_lstm_step_split16 / ASLP_LSTM_STEP_SPLIT_F16=1)
int g_step_split_override = -1;   // -1 = the environment decides
bool step_split_on() {
  static const int env = [] {   // "1" or "0" count as a choice
    const char *e = getenv("ASLP_LSTM_STEP_SPLIT_F16");
    return (e != nullptr && (e[0] == '0' || e[0] == '1') && e[1] == 0) ? e[0] - '0' : -1;
  }();
  if (g_step_split_override >= 0) return g_step_split_override != 0;
  if (env >= 0) return env != 0;
  return fp16_operands_on();
}
thread_local int t_step_last_pieces = 0;   // aslp_lstm_step_last_pieces()

void step_backward_cell(const aslp_lstm_step *a, const float *partial, int with_partial, const char *who) {
  dim3 grid(grid_for((long)a->S * a->C), a->ndir);
  if (a->cifg) hipLaunchKernelGGL((lstm_step_bwd_cell<true>), grid, dim3(kBlock), 0, cur_stream(), *a, partial, with_partial);
  else hipLaunchKernelGGL((lstm_step_bwd_cell<false>), grid, dim3(kBlock), 0, cur_stream(), *a, partial, with_partial);
  check_launch(who);
}
// scratch for the backward's K-split partial products (NULL with *with_partial set: the allocation failed)
float *step_partial_scratch(const aslp_lstm_step *a, int *with_partial) {
  *with_partial = 0;
  for (int d = 0; d < a->ndir; d++) *with_partial |= a->dir[d].has_next;
  if (!*with_partial) return nullptr;
  return static_cast<float *>(scratch(kScratchMisc, sizeof(float) * (size_t)a->ndir * kKQ * a->S * a->C));
}

}  // namespace
}  // namespace aslp

using namespace aslp;

extern "C" {

void aslp_lstm_step_split16(int on) { g_step_split_override = on < 0 ? -1 : (on != 0); }
int aslp_lstm_step_split16_get(void) { return step_split_on() ? 1 : 0; }
int aslp_lstm_step_last_pieces(void) { return t_step_last_pieces; }

void aslp_lstm_step_forward(const aslp_lstm_step *a) {
  if (!step_args_ok(a, "aslp_lstm_step_forward")) return;
  t_step_last_pieces = 0;
  dim3 grid((a->C + kCB - 1) / kCB, (a->S + 31) / 32, a->ndir);
  if (a->cifg) hipLaunchKernelGGL((lstm_step_fwd<true>), grid, dim3(64 * kNW), 0, cur_stream(), *a);
  else hipLaunchKernelGGL((lstm_step_fwd<false>), grid, dim3(64 * kNW), 0, cur_stream(), *a);
  check_launch("aslp_lstm_step_forward");
}

void aslp_lstm_step_backward(const aslp_lstm_step *a) {
  if (!step_args_ok(a, "aslp_lstm_step_backward")) return;
  t_step_last_pieces = 0;
  int with_partial = 0;
  float *partial = step_partial_scratch(a, &with_partial);
  if (with_partial) {
    if (!partial) return;
    dim3 grid((a->C + 31) / 32, kKQ * ((a->S + 31) / 32), a->ndir);
    if (a->cifg) hipLaunchKernelGGL((lstm_step_bwd_gemm<3>), grid, dim3(64 * kNW), 0, cur_stream(), *a, partial);
    else hipLaunchKernelGGL((lstm_step_bwd_gemm<4>), grid, dim3(64 * kNW), 0, cur_stream(), *a, partial);
  }
  step_backward_cell(a, partial, with_partial, "aslp_lstm_step_backward");
}

void aslp_lstm_step_forward_h(const aslp_lstm_step_h *ah) {
  if (!ah) { set_error("aslp_lstm_step_forward_h: bad arguments"); return; }
  if (!step_split_on()) { aslp_lstm_step_forward(&ah->step); return; }
  const aslp_lstm_step *a = &ah->step;
  const int np = aslp_lstm_operand_pieces_get() == 1 ? 1 : 2;
  if (!step_args_ok(a, "aslp_lstm_step_forward_h") || !step_planes_ok(ah, a->C, np, "aslp_lstm_step_forward_h")) return;
  t_step_last_pieces = np;
  dim3 grid((a->C + kCB - 1) / kCB, (a->S + 31) / 32, a->ndir), block(64 * kNW);
  if (a->cifg) {
    if (np == 1) hipLaunchKernelGGL((lstm_step_fwd_h<true, 1>), grid, block, 0, cur_stream(), *ah);
    else hipLaunchKernelGGL((lstm_step_fwd_h<true, 2>), grid, block, 0, cur_stream(), *ah);
  } else {
    if (np == 1) hipLaunchKernelGGL((lstm_step_fwd_h<false, 1>), grid, block, 0, cur_stream(), *ah);
    else hipLaunchKernelGGL((lstm_step_fwd_h<false, 2>), grid, block, 0, cur_stream(), *ah);
  }
  check_launch("aslp_lstm_step_forward_h");
}

void aslp_lstm_step_backward_h(const aslp_lstm_step_h *ah) {
  if (!ah) { set_error("aslp_lstm_step_backward_h: bad arguments"); return; }
  if (!step_split_on()) { aslp_lstm_step_backward(&ah->step); return; }
  const aslp_lstm_step *a = &ah->step;
  const int np = aslp_lstm_operand_pieces_get() == 1 ? 1 : 2;
  if (!step_args_ok(a, "aslp_lstm_step_backward_h")) return;
  int with_partial = 0;
  float *partial = step_partial_scratch(a, &with_partial);
  t_step_last_pieces = np;
  if (with_partial) {
    if (!partial || !step_planes_ok(ah, (a->cifg ? 3 : 4) * a->C, np, "aslp_lstm_step_backward_h")) return;
    dim3 grid((a->C + 31) / 32, kKQ * ((a->S + 31) / 32), a->ndir), block(64 * kNW);
    if (a->cifg) {
      if (np == 1) hipLaunchKernelGGL((lstm_step_bwd_gemm_h<3, 1>), grid, block, 0, cur_stream(), *ah, partial);
      else hipLaunchKernelGGL((lstm_step_bwd_gemm_h<3, 2>), grid, block, 0, cur_stream(), *ah, partial);
    } else {
      if (np == 1) hipLaunchKernelGGL((lstm_step_bwd_gemm_h<4, 1>), grid, block, 0, cur_stream(), *ah, partial);
      else hipLaunchKernelGGL((lstm_step_bwd_gemm_h<4, 2>), grid, block, 0, cur_stream(), *ah, partial);
    }
  }
  step_backward_cell(a, partial, with_partial, "aslp_lstm_step_backward_h");
}

}  // extern "C"
