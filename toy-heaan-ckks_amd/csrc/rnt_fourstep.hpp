// rnt_fourstep.hpp -- the radix-16 pass machinery of the four-step transform,
// shared by the units that run it: rnt_col.hip (column passes) and rnt_rows.hip
// (row passes and whole-plane products, key-switch rows, tensor rows).  Pass
// schedules and LDS geometries (RowGeo, ColGeo), the CT / GS pass templates, the occupancy bounds, and the host side
// of a row launch (LDS size, row-length dispatch).
//
// Transform: merged negacyclic Cooley-Tukey (twist folded into the
// twiddles: psi_rev[g] = psi^{brv(g)} over the heap g in [1, N)), output in
// bit-reversed order; inverse is the matching Gentleman-Sande network with
// n^-1 folded into its last stage.  Values equal the reference's
// a(psi^(2k+1)) exactly; only the order is private.
// Twiddles are stored interleaved with their Shoup companions ({w, w'}
// pairs) so one 8-byte load fetches both.
//
// Decomposition N = R * C (see rnt_internal.hpp):
//   column pass: stages with distance >= C, one column (stride C) per
//                thread, R <= 16 registers, coalesced 256 B per wave load;
//   row pass:    stages with distance < C, one row of C contiguous words per
//                C/16 threads, radix-16 register passes, LDS exchanges with a
//                1-in-16 pad (conflict-free for every pass distribution).
//                The row geometry is a template (RowGeo<LOG_C>): pass bit
//                ranges, LDS offsets and twiddle-subtree shapes are all
//                compile-time, so only one base address per thread is live.
#pragma once
#include "rnt_device.hpp"

namespace rnt {

// ---------------------------------------------------------------------------
// row passes
// ---------------------------------------------------------------------------

// Radix-16 pass schedule of one transform of length 2^LOGX held by T
// threads x E registers.  Passes run from the top bits down: full radix-16
// passes on bits [bb, bb+4), then (if LOGX % 4) a partial pass on bits
// [0, REM) with register bits [0, 4).  LOGX < 4: one thread holds it all.
template <int LOGX>
struct PassSched {
  static constexpr int LOGX_ = LOGX;
  static constexpr int LOGE = LOGX < 4 ? LOGX : 4;
  static constexpr int E = 1 << LOGE;
  static constexpr int LOG_T = LOGX - LOGE;
  static constexpr int T = 1 << LOG_T;
  static constexpr int X = 1 << LOGX;
  static constexpr int FULL = LOGX >= 4 ? LOGX / LOGE : 0;
  static constexpr int REM = LOGX >= 4 ? LOGX % LOGE : LOGX;
  static constexpr int P = FULL + (REM ? 1 : 0);
  static constexpr int bb(int p) { return (p >= 0 && p < FULL) ? LOGX - LOGE * (p + 1) : 0; }
  static constexpr int k(int p) { return p < FULL ? LOGE : REM; }
  static constexpr int BB0 = bb(0);
  static constexpr int BBL = bb(P - 1);
  // transform-local index of register i in the distribution with register
  // bits [b, b+LOGE): base(tau, b) | (i << b)
  __device__ static __forceinline__ uint32_t base(uint32_t tau, int b) {
    const uint32_t lowmask = (1u << b) - 1u;
    return (tau & lowmask) | ((tau >> b) << (b + LOGE));
  }
};

// Rows: RPW rows of C = 2^LOG_C contiguous words per workgroup; each row has
// its own LDS region with a 1-in-16 pad.  swz(base | (i<<b)) =
// swz(base) + (i<<b) + ((i<<b)>>4) because base has zero bits in [b, b+4).
template <int LOG_C>
struct RowGeo : PassSched<LOG_C> {
  using S = PassSched<LOG_C>;
  static constexpr int LOGC = LOG_C;
  static constexpr int C = 1 << LOG_C;
  // one pad word per 2^PADSH words (16 for the radix-16 passes)
  static constexpr int PADSH = S::LOGE == 3 ? 3 : 4;
  static constexpr int PADC = C + (C >> PADSH);
  static constexpr int THREADS = S::T > kRowThreads ? S::T : kRowThreads;
  static constexpr int RPW = THREADS / S::T;  // rows per workgroup
  static constexpr int REGION = RPW * PADC;   // LDS words per operand
  __device__ static __forceinline__ uint32_t slot_of(uint32_t tid) { return tid >> S::LOG_T; }
  __device__ static __forceinline__ uint32_t tau_of(uint32_t tid) { return tid & (S::T - 1); }
  __device__ static __forceinline__ uint32_t lds_off(uint32_t slot, uint32_t j) {
    return slot * PADC + j + (j >> PADSH);
  }
  static constexpr uint32_t lds_ioff(int i, int b) {
    return ((uint32_t)i << b) + (((uint32_t)i << b) >> PADSH);
  }
};

// Column tiles: TC = 2^LOG_TC adjacent columns of a stride-C, length-R
// column transform per workgroup; LDS is [j][TC] so consecutive lanes hit
// consecutive banks.  TC = 64 (C >= 64) makes a wave's 64 lanes one tau, so
// every twiddle a wave needs is wave-uniform: they come through scalar loads
// into SGPRs (no VGPRs, no vector memory ops); TC = 32 (C = 32) keeps them
// per-lane.
template <int LOG_R, int LOG_TC>
struct ColGeo : PassSched<LOG_R> {
  using S = PassSched<LOG_R>;
  static constexpr int LOGTC = LOG_TC;
  static constexpr int TC = 1 << LOG_TC;
  static constexpr bool UNIFORM = TC == 64;
  static constexpr int THREADS = TC * S::T;
  static constexpr int REGION = S::X * TC;
  __device__ static __forceinline__ uint32_t slot_of(uint32_t tid) { return tid & (TC - 1); }
  __device__ static __forceinline__ uint32_t tau_of(uint32_t tid) {
    if constexpr (UNIFORM) return __builtin_amdgcn_readfirstlane(tid >> LOG_TC);
    else return tid >> LOG_TC;
  }
  __device__ static __forceinline__ uint32_t lds_off(uint32_t slot, uint32_t j) {
    return j * TC + slot;
  }
  static constexpr uint32_t lds_ioff(int i, int b) { return ((uint32_t)i << b) * TC; }
};

// CT stages on bits [BB, BB+K) for NOPS operands sharing twiddles.  `node0`
// = heap index base of register 0: (heap root of this transform) * 2^LOGX +
// its transform-local index, so stage s's node is node0 >> (s+1) + (i >> ...).
// SLMIN > 0 stops SLMIN stages early (the truncated product transform); the
// last stage run then leaves its outputs canonical.
template <class W, int NOPS, int LOGE, int K, int BB, class TS, class MO, int SLMIN = 0>
__device__ __forceinline__ void pass_ct(W (&x)[NOPS][1 << LOGE], uint32_t node0, const TS& tw,
                                        const MO& mo) {
  constexpr int E = 1 << LOGE;
#pragma unroll
  for (int sl = K - 1; sl >= SLMIN; --sl) {
    constexpr int H = E > 1 ? E / 2 : 1;
    const int cnt = H >> sl;  // distinct twiddles at this stage
    const uint32_t nb = node0 >> (BB + sl + 1);
    Tw<W> t[H];
#pragma unroll
    for (int m = 0; m < H; ++m)
      if (m < cnt) t[m] = tw_get<W>(tw, nb, (uint32_t)m);
    const int d = 1 << sl;
#pragma unroll
    for (int i = 0; i < E; ++i) {
      if (i & d) continue;
      const int m = i >> (sl + 1);
      // inside a pass, outputs the next stage only multiplies stay unreduced
      const bool lazy = sl > SLMIN && (i & (d >> 1));
#pragma unroll
      for (int o = 0; o < NOPS; ++o) {
        if (lazy)
          ct_bfly_lazy(x[o][i], x[o][i | d], t[m].w, t[m].p, mo);
        else
          ct_bfly(x[o][i], x[o][i | d], t[m].w, t[m].p, mo);
      }
    }
  }
}

// GS stages; with FOLD the transform's top stage (bit LOGX-1, distance N/2
// of the whole network) applies the folded n^-1 constants instead.
template <class W, int NOPS, int LOGE, int K, int BB, int LOGX, bool FOLD, class TS, class MO,
          int SLMIN = 0>
__device__ __forceinline__ void pass_gs(W (&x)[NOPS][1 << LOGE], uint32_t node0, const TS& itw,
                                        const MO& mo, const Fold<W>& f) {
  const W bias = gs_bias(mo);
  constexpr int E = 1 << LOGE;
#pragma unroll
  for (int sl = SLMIN; sl < K; ++sl) {
    constexpr int H = E > 1 ? E / 2 : 1;
    const int d = 1 << sl;
    if (FOLD && BB + sl + 1 == LOGX) {
#pragma unroll
      for (int i = 0; i < E; ++i) {
        if (i & d) continue;
#pragma unroll
        for (int o = 0; o < NOPS; ++o) {
          const W u = x[o][i], v = x[o][i | d];
          x[o][i] = shoup_mul(u + v, f.c1, f.c1p, mo);
          x[o][i | d] = shoup_mul(u - v + bias, f.c2, f.c2p, mo);
        }
      }
      continue;
    }
    const int cnt = H >> sl;
    const uint32_t nb = node0 >> (BB + sl + 1);
    Tw<W> t[H];
#pragma unroll
    for (int m = 0; m < H; ++m)
      if (m < cnt) t[m] = tw_get<W>(itw, nb, (uint32_t)m);
#pragma unroll
    for (int i = 0; i < E; ++i) {
      if (i & d) continue;
      const int m = i >> (sl + 1);
#pragma unroll
      for (int o = 0; o < NOPS; ++o) gs_bfly(x[o][i], x[o][i | d], t[m].w, t[m].p, mo);
    }
  }
}

// Minimum resident waves per SIMD requested for the row kernels (caps their
// VGPR budget at 512 / kRowMinWaves) and for the key-switch rows.
constexpr int kRowMinWaves = 6;
// ... and for the whole-plane u32 rows (two operand planes of 16 registers,
// no spills at 128 VGPRs; the u64 rows are left unconstrained)
constexpr int kWholeMinWaves = 4;
// (RNT_KS_ROWS_WAVES: A/B builds of the four-step key-switch rows' bound)
#ifndef RNT_KS_ROWS_WAVES
#define RNT_KS_ROWS_WAVES 4
#endif
constexpr int kKsMinWaves = 4;
// Key rows of the key-switch rows kernel go global -> LDS directly
// (global_load_lds, no registers) for u32 rows of >= 64 words, except in the
// WIDE (small-batch) grid below 2^9-word rows, where staging them through
// registers measured faster (profiles/r02_ab_ks_small_batch.txt).
constexpr int kKsGldsWideMinLogC = 9;

// Move NOPS register sets from distribution BF to BT through LDS.  Several
// operands go one after the other through a single LDS region, so occupancy
// is bounded by VGPRs rather than LDS, at two barriers per operand.
template <class G, class W, int NOPS, int BF, int BT>
__device__ __forceinline__ void xchg(W (&x)[NOPS][G::E], W* lds, uint32_t slot, uint32_t tau) {
  const uint32_t wb = G::lds_off(slot, G::base(tau, BF));
  const uint32_t rb = G::lds_off(slot, G::base(tau, BT));
#pragma unroll
  for (int o = 0; o < NOPS; ++o) {
#pragma unroll
    for (int i = 0; i < G::E; ++i) lds[wb + G::lds_ioff(i, BF)] = x[o][i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < G::E; ++i) x[o][i] = lds[rb + G::lds_ioff(i, BT)];
    __syncthreads();
  }
}

// Per-thread transform coordinates: `slot` (which transform of the
// workgroup), `tau` (thread within it), `heap` (heap index of the
// transform's root times its length: node0 = heap + local index).
struct XPos {
  uint32_t slot, tau;
  uint32_t heap;
};

template <class G, class W, int NOPS, int PP, int SLMIN = 0, class TS, class MO>
__device__ __forceinline__ void fwd_pass(W (&x)[NOPS][G::E], const XPos& xp, W* lds, const TS& tw,
                                         const MO& q) {
  constexpr int BB = G::bb(PP);
  if constexpr (PP > 0) xchg<G, W, NOPS, G::bb(PP - 1), BB>(x, lds, xp.slot, xp.tau);
  pass_ct<W, NOPS, G::LOGE, G::k(PP), BB, TS, MO, SLMIN>(x, xp.heap + G::base(xp.tau, BB), tw, q);
}

template <class G, class W, int NOPS, int PP, bool FOLD, int SLMIN = 0, class TS, class MO>
__device__ __forceinline__ void inv_pass(W (&x)[NOPS][G::E], const XPos& xp, W* lds, const TS& itw,
                                         const MO& q, const Fold<W>& f) {
  constexpr int BB = G::bb(PP);
  if constexpr (PP < G::P - 1) xchg<G, W, NOPS, G::bb(PP + 1), BB>(x, lds, xp.slot, xp.tau);
  pass_gs<W, NOPS, G::LOGE, G::k(PP), BB, G::LOGX_, FOLD, TS, MO, SLMIN>(
      x, xp.heap + G::base(xp.tau, BB), itw, q, f);
}

// All forward passes (first-pass distribution in, last-pass out).
template <class G, class W, int NOPS, class TS, class MO>
__device__ __forceinline__ void xf_fwd(W (&x)[NOPS][G::E], const XPos& xp, W* lds, const TS& tw,
                                       const MO& q) {
  if constexpr (G::P > 0) fwd_pass<G, W, NOPS, 0>(x, xp, lds, tw, q);
  if constexpr (G::P > 1) fwd_pass<G, W, NOPS, 1>(x, xp, lds, tw, q);
  if constexpr (G::P > 2) fwd_pass<G, W, NOPS, 2>(x, xp, lds, tw, q);
  if constexpr (G::P > 3) fwd_pass<G, W, NOPS, 3>(x, xp, lds, tw, q);
}

// All inverse passes (last-pass distribution in, first-pass out).
template <class G, class W, int NOPS, bool FOLD = false, class TS, class MO>
__device__ __forceinline__ void xf_inv(W (&x)[NOPS][G::E], const XPos& xp, W* lds, const TS& itw,
                                       const MO& q, const Fold<W>& f = Fold<W>{}) {
  if constexpr (G::P > 3) inv_pass<G, W, NOPS, 3, FOLD>(x, xp, lds, itw, q, f);
  if constexpr (G::P > 2) inv_pass<G, W, NOPS, 2, FOLD>(x, xp, lds, itw, q, f);
  if constexpr (G::P > 1) inv_pass<G, W, NOPS, 1, FOLD>(x, xp, lds, itw, q, f);
  if constexpr (G::P > 0) inv_pass<G, W, NOPS, 0, FOLD>(x, xp, lds, itw, q, f);
}

// Row coordinates of this thread.
struct RowPos {
  XPos xp;
  uint32_t l, p, r;
  bool active;
};

// Row coordinates with the poly index fastest: row = ((l * R + r) * B + p).
// Consecutive rows of a workgroup then share (limb, row r), so whatever they
// read per (limb, r) -- gadget-key rows, twiddles -- is fetched from HBM once
// and hit in cache by the rest of the batch.
template <class G>
__device__ __forceinline__ RowPos row_pos_pfast(uint32_t log_n, uint32_t B, uint64_t rows_total) {
  RowPos rp;
  rp.xp.slot = G::slot_of(threadIdx.x);
  rp.xp.tau = G::tau_of(threadIdx.x);
  uint64_t row = (uint64_t)blockIdx.x * G::RPW + rp.xp.slot;
  rp.active = row < rows_total;
  if (!rp.active) row = 0;
  const uint32_t log_r = log_n - G::LOGC;
  const uint64_t lr = row / B;
  rp.p = (uint32_t)(row - lr * B);
  rp.r = (uint32_t)(lr & ((1u << log_r) - 1u));
  rp.l = (uint32_t)(lr >> log_r);
  rp.xp.heap = (1u << log_n) + rp.r * (uint32_t)G::C;  // (R + r) * C
  return rp;
}

#define RNT_DISPATCH_LOGC(LOGC, MACRO) \
  switch (LOGC) {                      \
    case 0: MACRO(0);                  \
    case 1: MACRO(1);                  \
    case 2: MACRO(2);                  \
    case 3: MACRO(3);                  \
    case 4: MACRO(4);                  \
    case 5: MACRO(5);                  \
    case 6: MACRO(6);                  \
    case 7: MACRO(7);                  \
    case 8: MACRO(8);                  \
    case 9: MACRO(9);                  \
    default: return hipErrorInvalidValue; \
  }

template <class W, int LOG_C>
static size_t row_lds(int nops) {
  using G = RowGeo<LOG_C>;
  (void)nops;  // operands share one region (xchg)
  return (size_t)G::RPW * G::PADC * sizeof(W);
}

// u32 bases only: the u64 form needs 256 VGPRs (one wave per SIMD).
// N <= 2^13: at 2^14 (one 1024-thread workgroup per plane, one per CU)
// the whole-plane tensor and key-switch measured slower than the four-step
// kernels at every batch but 32 (ct-mul 2^14 x 8: 97.1k vs 99.1k/s at 1024
// cts, 3.3k vs 4.5k/s at one), faster at every batch at 2^10..2^13
// (profiles/r04/ab_ks_whole.txt)
constexpr uint32_t kKsWholeMaxLogN = 13;
}  // namespace rnt
