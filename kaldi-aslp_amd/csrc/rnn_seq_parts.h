// rnn_seq_parts.h -- the parts the persistent recurrence kernels of rnn_persistent.hip share.
//  * File scope (LSTM and GRU): SeqStatus and the phase timers, the bounded spin (spin_ok), buffer descriptors and the sentinel test, the DPP
//    moves, store_tile16, the chain constants with ChainRole / chain_role, the gate non-linearities with their derivatives.  Moving these here
//    left the compiler's output for all 42 kernels of that translation unit identical.
//  * Parts of an LSTM timestep that the two kernels of a pass (fp32 product / fp16 product) instantiate from ONE copy here: forward the W_first
//    staging and the r(0) staging, backward the gate-block derivatives.  Each takes scalars and pointers only, and with them the compiler's
//    output for all 42 kernels is still identical to what the verbatim copies gave, instruction for instruction.
//  * Two more, which keep every kernel's resource table (SGPRs, VGPRs, AGPRs, scratch, spills, LDS, occupancy: profiles/lstm_seq_parts_resources.txt)
//    but change the instruction text of the LSTM kernels: reading the fail[] vote (seq_failed: all 36 LSTM kernels and, text unchanged, the GRU
//    kernels) and the step-0 product (fwd_first_product, 24 kernels).  They take scalars, pointers and references to register arrays; aslp_lstm_seq,
//    aslp_lstm_seq_dir or ChainRole handed on by reference move register counts.  Only the vote is on the per-timestep path.  Checked on the GPU
//    against the copies: devtools/lstm_seq_sweep.py writes the same file (profiles/lstm_seq_sweep.txt, to cmp the next change against); the cfg3
//    step is inside the old build's run-to-run distance in 9 of 9 (default path) and 6 of 9 (fp32 instruction) runs old / new / old (profiles/lstm_seq_parts_timing.txt).
// What is still a copy in every kernel moved a resource count when taken out alone: see the one-line notes at those places in rnn_persistent.hip
// (the hand-off waits, posting into fail[], the red[] store, the forward gate block, the backward stores and sums, the tail, and -- each tried on
// its own as a function returning a small record -- the role / geometry prologue and the backward loads).  The grad_partial reduction behind the
// backward loop keeps the table as a function but not the bits: the compiler then forms other FMAs in the time loop of lstm_seq_bwd
// (note there; profiles/lstm_seq_grad_partial_as_function.txt).
// This header defines a __shared__ array (g_tacc) and lives in an anonymous namespace: it is meant for ONE translation unit, rnn_persistent.hip.
#pragma once
#include "aslp_kernels.h"
#include "common.h"

namespace aslp {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr unsigned kSentinel = 0xFFFFFFFFu;
constexpr int kAuxSc1 = 16;          // buffer instruction cache policy: sc1 = agent scope
constexpr long kSpinLimitTicks = 200000000L;  // wall_clock64 runs at 100 MHz: 2 s

__device__ __forceinline__ float dsigm(float y, float d) { return d * y * (1.0f - y); }
__device__ __forceinline__ float dtanh(float y, float d) { return d * (1.0f - y * y); }

// Every base pointer handed to a buffer instruction here is wave-uniform by construction (kernel arguments, blockIdx, the loop
// counter), but hipcc cannot always prove it (the direction's pointers are picked from the argument struct with an index that
// went through shared memory) and then wraps EVERY buffer load / store in a waterfall loop over the lanes' descriptor values.
// readfirstlane makes the uniformity explicit: the descriptor lives in SGPRs and the access is one instruction.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const float *p) {
  const unsigned long long v = reinterpret_cast<unsigned long long>(p);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  float *u = reinterpret_cast<float *>(((unsigned long long)hi << 32) | lo);
  return __builtin_amdgcn_make_buffer_rsrc(u, 0, 0x7fffffff, 0x00020000);
}
__device__ __forceinline__ bool has_sentinel(const u32x4 &v) {
  return v.x == kSentinel || v.y == kSentinel || v.z == kSentinel || v.w == kSentinel;
}
__device__ __forceinline__ float as_f(unsigned u) { return __uint_as_float(u); }
// cross-lane moves on the DPP path of the VALU (no LDS crossbar round trip like ds_bpermute): lane K of the caller's quad, and the
// lane N places up within the caller's row of 16 lanes
template <int K>
__device__ __forceinline__ float quad_bcast(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), K * 0x55, 0xF, 0xF, true));   // quad_perm:[K,K,K,K]
}
template <int N>
__device__ __forceinline__ float row_up(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x100 + N, 0xF, 0xF, true));  // row_shl:N -> dst[i] = src[i + N]
}

template <int N>
__device__ __forceinline__ float row_ror(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x120 + N, 0xF, 0xF, true));  // row_ror:N -> rotation within the row of 16 lanes
}

// device-side status: abort_flag[0] abort flag (zeroed before every launch), abort_flag[2] running count of hand-off
// re-polls (diagnostics, aslp_lstm_seq_polls); host_err: mapped host word, counts timeouts
struct SeqStatus {
  unsigned *abort_flag;
  unsigned *host_err;
  unsigned long long *timing;  // diagnostics (devtools): NULL, or 8 accumulators of 10 ns ticks written by workgroup 0, wave 0
  unsigned long long *trace;   // diagnostics (devtools): NULL, or [workgroup][2] entry / exit clock of the latest launch
  unsigned epoch;              // launch counter (28 bits, never 0): tags the placement table entries of this launch
  unsigned wave_collect;       // LSTM forward.  bit 0: every wave collects the K slice of m(t-1) it multiplies itself (no workgroup barrier behind the
                               // collection); bit 1: operand reads pinned four fragments ahead of the products
};
__device__ __forceinline__ long tick(const SeqStatus &st) { return st.timing ? (long)wall_clock64() : 0; }
// The phase accumulators live in LDS while the kernel runs (a fire-and-forget ds_add per mark): accumulating in global memory put an L2
// round trip and a wait behind every mark -- 0.1-0.2 us charged to the NEXT phase, five times per timestep, and workgroup 0 (hence the
// whole lock-stepped chain) ran that much slower under the timer.  timing_flush adds them to st.timing once, at the end.
__shared__ unsigned long long g_tacc[8];
__device__ __forceinline__ void timing_begin(const SeqStatus &st) {
  if (st.timing && threadIdx.x < 8) g_tacc[threadIdx.x] = 0ull;   // (chain_role's barrier publishes it)
}
__device__ __forceinline__ void timing_flush(const SeqStatus &st) {   // caller: st.timing != NULL, workgroup 0, thread 0, behind the loop's last barrier
  for (int k = 1; k <= 5; k++) st.timing[k] += g_tacc[k];
}
__device__ __forceinline__ void tock(const SeqStatus &st, int slot, long &t) {
  if (!st.timing) return;
  const long now = (long)wall_clock64();
  if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_fetch_add(&g_tacc[slot], (unsigned long long)(now - t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  t = now;
}

// the same for the first thread of the gate role (thread 256) of the wave-specialised kernel
__device__ __forceinline__ void tock_gate(const SeqStatus &st, int slot, long &t) {
  if (!st.timing) return;
  const long now = (long)wall_clock64();
  if (blockIdx.x == 0 && threadIdx.x == 256) __hip_atomic_fetch_add(&g_tacc[slot], (unsigned long long)(now - t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  t = now;
}

// Bounded spin bookkeeping shared by the two phases below: false = give up (device-wide abort or 2 s without progress).
__device__ __forceinline__ bool spin_ok(unsigned spins, long &t0, const SeqStatus &st) {
  if ((spins & 31u) != 31u) return true;
  if (__hip_atomic_load(st.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return false;
  const long now = (long)wall_clock64();
  if (t0 == 0) { t0 = now; return true; }
  if (now - t0 <= kSpinLimitTicks) return true;
  if ((threadIdx.x & 63) == 0) {
    __hip_atomic_store(st.abort_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(st.host_err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  return false;
}

// The workgroup's vote behind a barrier: did one of its 8 waves give up in this round (spin_ok)?  Uniform: every wave reads the same eight words.
__device__ __forceinline__ bool seq_failed(const int (*fail)[8], int round) {
  int f = 0;
#pragma unroll
  for (int w = 0; w < 8; w++) f |= fail[round][w];
  return f != 0;
}

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
// C/D layout of v_mfma_f32_16x16x4_f32: element e of lane l is row 4 * (l >> 4) + e, column l & 15
constexpr int kTP = 17;  // LDS pitch of a 16 x 16 partial tile
__device__ __forceinline__ void store_tile16(float *tile, const f32x4 &acc, int lane) {
  const int n = lane & 15, r0 = 4 * (lane >> 4);
  tile[(r0 + 0) * kTP + n] = acc.x;
  tile[(r0 + 1) * kTP + n] = acc.y;
  tile[(r0 + 2) * kTP + n] = acc.z;
  tile[(r0 + 3) * kTP + n] = acc.w;
}

// ---- chain geometry shared by both kernels ------------------------------------------------------------------------
constexpr int kFirstK = 256;       // largest K of a first-step product served inside the forward launch (aslp_lstm_seq_dir.w_first)
constexpr int kChainStreams = 8;   // streams per chain (rows 0..7 of the 16-row MFMA tile; rows 8..15 repeat them, outputs unused)
constexpr int kCellsPerWg = 16;
constexpr int kMaxChains = 8;      // = XCDs of the chip: workgroup b serves chain b & 7
constexpr int kMaxWgPerChain = 32; // = CUs of one XCD (C <= 512)

struct ChainRole {
  int dir, s0, c0;   // direction, first stream, first cell
  bool active;       // this workgroup has a chain to serve
  bool local;        // the chain's workgroups share one XCD (one L2): plain stores suffice
};

// Who am I, and does my chain sit on one XCD?  place: [kMaxChains][kMaxWgPerChain] words; an entry counts once it carries
// this launch's epoch (a host-side launch counter, st.epoch) -- nothing to clear between launches.
__device__ __forceinline__ ChainRole chain_role(int S, int ndir, int C, const SeqStatus &st, unsigned *place, int *lds_flag) {
  ChainRole r;
  const int chain = blockIdx.x & (kMaxChains - 1), cb = blockIdx.x >> 3;
  const int nsg = (S + kChainStreams - 1) / kChainStreams, nchains = ndir * nsg, wpc = (C + kCellsPerWg - 1) / kCellsPerWg;
  r.active = chain < nchains;
  r.dir = r.active ? chain % ndir : 0;
  r.s0 = (r.active ? chain / ndir : 0) * kChainStreams;
  r.c0 = cb * kCellsPerWg;
  r.local = false;
  if (!r.active) return r;
  if (threadIdx.x < 64) {  // wave 0
    unsigned xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    xcc = (xcc & 15u) | (st.epoch << 4);  // entries of earlier launches carry another epoch = "not yet written"
    unsigned *row = place + chain * kMaxWgPerChain;
    if (threadIdx.x == 0) __hip_atomic_store(row + cb, xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int l = threadIdx.x;
    unsigned v = xcc;
    long t0 = 0;
    bool ok = true;
    for (unsigned spins = 0;; spins++) {
      if (l < wpc) v = __hip_atomic_load(row + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (!__any(l < wpc && (v >> 4) != st.epoch)) break;
      if (!spin_ok(spins, t0, st)) { ok = false; break; }
      __builtin_amdgcn_s_sleep(4);
    }
    const bool same = __all(l >= wpc || v == xcc);
    if (threadIdx.x == 0) *lds_flag = !ok ? -1 : (same ? 1 : 0);
  }
  __syncthreads();
  const int f = *lds_flag;
  if (f < 0) r.active = false;  // timed out waiting for the chain to show up: abort word is set, leave
  r.local = f == 1;
  return r;
}

// The gate non-linearities on the hardware's exp2 and reciprocal (v_exp_f32, v_rcp_f32: 1 ulp each) instead of the correctly rounded
// expf and division of sigmoid_ref / tanh_ref: ~6 instructions on the sequential path of a timestep instead of ~60, results within a
// few ulp (1e-6 relative after T = 60 steps; the parity bar is 1e-4).  Default; ASLP_LSTM_FAST_ACT=0 keeps the exact forms (A/B).
template <bool FAST>
__device__ __forceinline__ float act_sigmoid(float x) {
  if (!FAST) return sigmoid_ref(x);
  const float e = __builtin_amdgcn_exp2f(-1.44269504088896340736f * fabsf(x));
  return (x > 0.0f ? 1.0f : e) * __builtin_amdgcn_rcpf(1.0f + e);
}
template <bool FAST>
__device__ __forceinline__ float act_tanh(float x) {
  if (!FAST) return tanh_ref(x);
  const float e2 = __builtin_amdgcn_exp2f(-2.88539008177792681472f * fabsf(x));   // exp(-2 |x|)
  const float q = 2.0f * __builtin_amdgcn_rcpf(1.0f + e2);
  return x > 0.0f ? -1.0f + q : 1.0f - q;
}

// ---- parts of an LSTM timestep, one copy for the two kernels of a pass (scalars and pointers only: see the top of this file) -------------
// backward: the gate-block derivatives of one (stream, cell) pair; dn_*: the own-cell terms of the step processed just before
struct BwdDiffs { float dh, dov, dc, dg, df, di; };
template <bool CIFG>
__device__ __forceinline__ BwdDiffs bwd_gate_diffs(float dm, float yo, float yh, float yg, float yf, float yi, float yn_f, float cprev, float dn_c, float dn_f,
                                                   float dn_i, float pf, float po, float pi) {
  const float dh = dtanh(yh, dm * yo);
  const float dov = dsigm(yo, dm * yh);
  float dc = dh + dn_c * yn_f;
  if (!CIFG) dc += dn_i * pi;
  dc += dn_f * pf;
  dc += dov * po;
  float dg, df, di = 0.f;
  if (!CIFG) {
    df = dsigm(yf, dc * cprev);
    di = dsigm(yi, dc * yg);
    dg = dtanh(yg, dc * yi);
  } else {
    df = dsigm(yf, dc * cprev - dc * yg);
    dg = dtanh(yg, dc - dc * yf);
  }
  return BwdDiffs{dh, dov, dc, dg, df, di};
}
// forward: W_first rows of this workgroup's 64 gate columns -> LDS (zero where the column or k does not exist); read at step 0 only
template <int G>
__device__ __forceinline__ void fwd_stage_w_first(float (*wf_lds)[kFirstK + 4], const float *w_first, int ldw_first, int k_first, int C, int c0) {
  const int kq = (k_first + 3) >> 2;   // 16-byte pieces per row
  for (int p = threadIdx.x; p < 64 * kq; p += 512) {
    const int n = p / kq, k0 = 4 * (p % kq), gate = n >> 4, cellb = c0 + (n & 15);
    const bool ok = gate < G && cellb < C;
    *reinterpret_cast<f32x4 *>(&wf_lds[n][k0]) = ok ? *reinterpret_cast<const f32x4 *>(w_first + (long)(gate * C + cellb) * ldw_first + k0)
                                                    : f32x4{0.f, 0.f, 0.f, 0.f};
  }
}
// forward: r(0) of the chain's streams -> LDS (the history row block: stored before the launch, no hand-off)
template <int MP>
__device__ __forceinline__ void fwd_stage_r0(float (*m_lds)[MP], const float *y, int col_first, int k_first, int tp, int S, int ld, int s0, int SE) {
  const int kq = k_first >> 2;
  for (int p = threadIdx.x; p < kChainStreams * kq; p += 512) {
    const int sp = p / kq, k0 = 4 * (p % kq);
    *reinterpret_cast<f32x4 *>(&m_lds[sp][k0]) =
        *reinterpret_cast<const f32x4 *>(y + ((long)tp * S + min(s0 + sp, SE - 1)) * ld + col_first + k0);
  }
}
// forward, step 0 with a W_first operand: r(0) W_first^T on v_mfma_f32_4x4x1, both operands from LDS (fwd_stage_r0, fwd_stage_w_first); this wave's
// slice of K = k_first.  Result register r of a lane = stream 4 qs + r of tile column 32 h + 4 qc + jl, even / odd k in acc[h][0] / acc[h][1].
template <int MP>
__device__ __forceinline__ void fwd_first_product(f32x4 (&acc)[2][2], const float (*m_lds)[MP], const float (*wf_lds)[kFirstK + 4], int k_first, int wave, int qs,
                                                  int qc, int jl) {
  const int kwf = ((k_first + 31) / 32) * 4, kbf = wave * kwf;
  const float *arow = &m_lds[4 * qs + jl][0];
  for (int k0 = kbf; k0 < min(kbf + kwf, k_first); k0 += 4) {
    const f32x4 av = *reinterpret_cast<const f32x4 *>(arow + k0);
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const f32x4 b = *reinterpret_cast<const f32x4 *>(&wf_lds[32 * h + 4 * qc + jl][k0]);
      acc[h][0] = __builtin_amdgcn_mfma_f32_4x4x1f32(av.x, b.x, acc[h][0], 0, 0, 0);
      acc[h][1] = __builtin_amdgcn_mfma_f32_4x4x1f32(av.y, b.y, acc[h][1], 0, 0, 0);
      acc[h][0] = __builtin_amdgcn_mfma_f32_4x4x1f32(av.z, b.z, acc[h][0], 0, 0, 0);
      acc[h][1] = __builtin_amdgcn_mfma_f32_4x4x1f32(av.w, b.w, acc[h][1], 0, 0, 0);
    }
  }
}

}  // namespace
}  // namespace aslp
