// rnt_col.hip -- the column passes of the four-step transform
// (rnt_fourstep.hpp) and their launchers: k_col_* (log2 R <= 4, one column a
// thread), k_colt_* (tiled through LDS), and the key-switch decompositions
// k_ks_decompose / k_colt_decompose fused with a forward column pass.
//
// Reference behaviour being replaced (oiwn/toy-heaan-ckks):
//   to_ntt_domain / to_coeff_domain   src/rings/backends/rns_ntt/poly.rs:136-166
//   forward_ntt / inverse_ntt / CT    poly.rs:574-625
//   gadget decomposition              src/crypto/engine.rs:507-516
#include <hip/hip_runtime.h>

#include "rnt_fourstep.hpp"
#include "rnt_launch.hpp"

namespace rnt {

Geom geom_for(uint32_t log_n) {
  Geom g;
  g.log_n = log_n;
  if (log_n < 4) {  // tiny rings: one row holds the whole polynomial
    g.log_r = 0;
    g.log_c = log_n;
  } else if (log_n < 8) {
    g.log_r = log_n - 4;
    g.log_c = 4;
  } else {
    // balance the stages between the (memory-bound) column passes and the
    // (ALU-bound) row pass: R = 2^floor(log_n / 2), at least 16
    g.log_r = log_n / 2 > 4 ? log_n / 2 : 4;
    g.log_c = log_n - g.log_r;
  }
  g.n = (size_t)1 << log_n;
  g.r = (size_t)1 << g.log_r;
  g.c = (size_t)1 << g.log_c;
  return g;
}

// ---------------------------------------------------------------------------
// column passes
// ---------------------------------------------------------------------------

template <class W, int LOG_R>
__device__ __forceinline__ void col_ct(W (&x)[1 << LOG_R], const Tw<W>* tw, const Mod<W>& m) {
  constexpr int R = 1 << LOG_R;
#pragma unroll
  for (int k = 0; k < LOG_R; ++k) {
    const int d = R >> (k + 1);
#pragma unroll
    for (int i = 0; i < R; ++i) {
      if (i & d) continue;
      const Tw<W> t = tw[(1 << k) + (i >> (LOG_R - k))];
      // outputs that the next stage only multiplies stay unreduced
      if (k + 1 < LOG_R && (i & (d >> 1)))
        ct_bfly_lazy<W>(x[i], x[i + d], t.w, t.p, m);
      else
        ct_bfly<W>(x[i], x[i + d], t.w, t.p, m);
    }
  }
}

// x <- GS network over the column with the last (distance N/2) stage scaled
// by c1 (upper) and c2 (lower).
template <class W, int LOG_R>
__device__ __forceinline__ void col_gs(W (&x)[1 << LOG_R], const Tw<W>* itw, const Mod<W>& m,
                                       W c1, W c1p, W c2, W c2p) {
  const W q = m.q;
  constexpr int R = 1 << LOG_R;
#pragma unroll
  for (int sl = 0; sl < LOG_R; ++sl) {
    const int d = 1 << sl;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      if (i & d) continue;
      if (sl == LOG_R - 1) {
        W u = x[i], v = x[i + d];
        x[i] = shoup_mul<W>(u + v, c1, c1p, m);
        x[i + d] = shoup_mul<W>(u - v + q, c2, c2p, m);
      } else {
        const Tw<W> t = itw[(1 << (LOG_R - 1 - sl)) + (i >> (sl + 1))];
        gs_bfly<W>(x[i], x[i + d], t.w, t.p, m);
      }
    }
  }
  if (LOG_R == 0) x[0] = shoup_mul<W>(x[0], c1, c1p, m);
}

// Forward column pass.  Thread = (limb l, poly p, column j1); j1 fastest.
// Operand 1 is processed first: out0 may alias in1 (out = a * b, out == b).
template <class W, int LOG_R>
__global__ void __launch_bounds__(256)
k_col_fwd(W* out0, const W* in0, W* out1, const W* in1, TabPtrs<W> tp, uint32_t log_n,
          uint32_t log_c, uint32_t B, uint64_t in_ls, uint64_t out_ls, uint64_t total) {
  const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= total) return;
  constexpr int R = 1 << LOG_R;
  const uint32_t C = 1u << log_c;
  const uint64_t N = 1ull << log_n;
  const uint32_t j1 = (uint32_t)(gid & (C - 1));
  const uint64_t lp = gid >> log_c;
  const uint32_t l = (uint32_t)(lp / B);
  const uint32_t p = (uint32_t)(lp - (uint64_t)l * B);
  const uint64_t ib = (uint64_t)l * in_ls + (uint64_t)p * N + j1;
  const uint64_t ob = (uint64_t)l * out_ls + (uint64_t)p * N + j1;
  const Mod<W> m = mod_of(tp.lc[l]);
  const Tw<W>* tw = tp.tw + (uint64_t)l * N;
  W x[R];
  if (in1 != nullptr) {
#pragma unroll
    for (int i = 0; i < R; ++i) x[i] = in1[ib + (uint64_t)i * C];
    col_ct<W, LOG_R>(x, tw, m);
#pragma unroll
    for (int i = 0; i < R; ++i) out1[ob + (uint64_t)i * C] = x[i];
  }
#pragma unroll
  for (int i = 0; i < R; ++i) x[i] = in0[ib + (uint64_t)i * C];
  col_ct<W, LOG_R>(x, tw, m);
#pragma unroll
  for (int i = 0; i < R; ++i) out0[ob + (uint64_t)i * C] = x[i];
}

template <class W, int LOG_R>
__global__ void __launch_bounds__(256)
k_col_inv(W* out, const W* in, const W* addend, TabPtrs<W> tp, uint32_t log_n, uint32_t log_c,
          uint32_t B, uint64_t in_ls, uint64_t out_ls, uint64_t total, int rfold) {
  const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= total) return;
  constexpr int R = 1 << LOG_R;
  const uint32_t C = 1u << log_c;
  const uint64_t N = 1ull << log_n;
  const uint32_t j1 = (uint32_t)(gid & (C - 1));
  const uint64_t lp = gid >> log_c;
  const uint32_t l = (uint32_t)(lp / B);
  const uint32_t p = (uint32_t)(lp - (uint64_t)l * B);
  const uint64_t ib = (uint64_t)l * in_ls + (uint64_t)p * N + j1;
  const uint64_t base = (uint64_t)l * out_ls + (uint64_t)p * N + j1;
  const LimbConst<W> lc = tp.lc[l];
  const Tw<W>* itw = tp.itw + (uint64_t)l * N;
  W x[R];
#pragma unroll
  for (int i = 0; i < R; ++i) x[i] = in[ib + (uint64_t)i * C];
  if (rfold == 2)
    col_gs<W, LOG_R>(x, itw, mod_of(lc), lc.c1t, lc.c1t_p, lc.c2t, lc.c2t_p);
  else if (rfold)
    col_gs<W, LOG_R>(x, itw, mod_of(lc), lc.c1r, lc.c1r_p, lc.c2r, lc.c2r_p);
  else
    col_gs<W, LOG_R>(x, itw, mod_of(lc), lc.c1, lc.c1_p, lc.c2, lc.c2_p);
  if (addend != nullptr) {
#pragma unroll
    for (int i = 0; i < R; ++i) x[i] = add_mod<W>(x[i], addend[base + (uint64_t)i * C], lc.q);
  }
#pragma unroll
  for (int i = 0; i < R; ++i) out[base + (uint64_t)i * C] = x[i];
}

// Key-switch decomposition + forward column pass (engine.rs:507-516 fused
// with the first half of alpha_i's forward NTT): thread = (target limb j,
// source limb i, poly p, column j1); reads limb i of d, reduces mod q_j
// canonically (R5), transforms with q_j's tables, writes S[j][i][p].
template <class W, int LOG_R>
__global__ void __launch_bounds__(256)
k_ks_decompose(W* __restrict__ S, const W* __restrict__ d, TabPtrs<W> tp, uint32_t log_n,
               uint32_t log_c, uint32_t L, uint32_t B, uint64_t d_ls, uint64_t total) {
  const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= total) return;
  constexpr int R = 1 << LOG_R;
  const uint32_t C = 1u << log_c;
  const uint64_t N = 1ull << log_n;
  const uint32_t j1 = (uint32_t)(gid & (C - 1));
  uint64_t rest = gid >> log_c;  // ((j*L + i)*B + p), L = source limbs
  const uint32_t p = (uint32_t)(rest % B);
  rest /= B;
  const uint32_t i = (uint32_t)(rest % L);
  const uint32_t j = (uint32_t)(rest / L);
  const LimbConst<W> lc = tp.lc[j];
  const Tw<W>* tw = tp.tw + (uint64_t)j * N;
  const uint64_t src = (uint64_t)i * d_ls + (uint64_t)p * N + j1;
  const uint64_t dst = (((uint64_t)j * L + i) * B + p) * N + j1;
  W x[R];
#pragma unroll
  for (int t = 0; t < R; ++t) x[t] = shoup_mul<W>(d[src + (uint64_t)t * C], (W)1, lc.one_p, lc.q);
  col_ct<W, LOG_R>(x, tw, mod_of(lc));
#pragma unroll
  for (int t = 0; t < R; ++t) S[dst + (uint64_t)t * C] = x[t];
}

// ---------------------------------------------------------------------------
// tiled column passes (log2 R >= 5): a workgroup owns TC = 32 adjacent
// columns of one (limb, poly) and runs the R-point network over the row
// index j (stride C) through LDS.  The column transform is the top of the
// heap: node0 = R + j.  Output stays in place (row j, column c).
// ---------------------------------------------------------------------------

struct ColPos {
  XPos xp;
  uint32_t l, p;
  uint32_t col;
};

// Grid: x = poly * (C / TC) + column tile, y = limb (no integer division,
// so limb and poly stay in SGPRs and the buffer descriptors built from them
// are provably wave-uniform).
template <class G>
__device__ __forceinline__ ColPos col_pos(uint32_t log_c) {
  ColPos cp;
  cp.xp.slot = G::slot_of(threadIdx.x);
  cp.xp.tau = G::tau_of(threadIdx.x);
  const uint32_t tpp_log = log_c - G::LOGTC;  // column tiles per (limb, poly)
  cp.l = blockIdx.y;
  cp.p = blockIdx.x >> tpp_log;
  const uint32_t ct = blockIdx.x & ((1u << tpp_log) - 1);
  cp.col = (ct << G::LOGTC) + cp.xp.slot;
  cp.xp.heap = (uint32_t)G::X;
  return cp;
}

// Per-lane element offset of register 0 and the wave-uniform register
// stride of a column tile in distribution bits [BB, BB+LOGE).
template <class G, int BB>
struct ColAddr {
  uint32_t v, s;
  __device__ ColAddr(const ColPos& cp, uint32_t log_c)
      : v(cp.col + (G::base(cp.xp.tau, BB) << log_c)), s(1u << (log_c + BB)) {}
  // Opaque redefinition of the stride: stops the compiler from keeping all
  // E soffsets (i * s) live across a transform, which spills them to VGPRs
  // and turns every buffer op into a waterfall loop.
  __device__ __forceinline__ void refresh() { asm volatile("" : "+s"(s)); }
};

template <class W, int LOG_R, int LOG_TC, bool LZ = false>
__global__ void __launch_bounds__((ColGeo<LOG_R, LOG_TC>::THREADS))
k_colt_fwd(W* out0, const W* in0, W* out1, const W* in1, TabPtrs<W> tp, uint32_t log_n,
           uint32_t log_c, uint32_t B, uint64_t in_ls, uint64_t out_ls) {
  using G = ColGeo<LOG_R, LOG_TC>;
  constexpr int E = G::E;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  W* lds = (W*)smem_raw;
  const ColPos cp = col_pos<G>(log_c);
  const uint32_t N = 1u << log_n;
  const uint64_t ip = (uint64_t)cp.l * in_ls + (uint64_t)cp.p * N;
  const uint64_t op = (uint64_t)cp.l * out_ls + (uint64_t)cp.p * N;
  ColAddr<G, G::BB0> a0(cp, log_c);
  ColAddr<G, G::BBL> al(cp, log_c);
  const auto tw = col_twiddles<W, G::UNIFORM>(tp.tw + (uint64_t)cp.l * N, N);
  const auto m = mod_for<W, LZ>(tp.lc[cp.l]);  // LZ: outputs in [0, 4q)
  W x[1][E];
  const BufView<W> src(in0 + ip, N), dst(out0 + op, N);
  // operand 1 first: out0 may alias in1 (out = a * b with out == b).  With
  // wave-uniform twiddles the registers are cheap, so operand 0's loads are
  // issued up front and land while operand 1 is transformed.
  if (in1 != nullptr) {
    const BufView<W> src1(in1 + ip, N), dst1(out1 + op, N);
    W y[1][E];
#pragma unroll
    for (int i = 0; i < E; ++i) y[0][i] = src1.ld(a0.v, i * a0.s);
    if constexpr (G::UNIFORM) {
#pragma unroll
      for (int i = 0; i < E; ++i) x[0][i] = src.ld(a0.v, i * a0.s);
    }
    xf_fwd<G, W, 1>(y, cp.xp, lds, tw, m);
#pragma unroll
    for (int i = 0; i < E; ++i) dst1.st(y[0][i], al.v, i * al.s);
    a0.refresh();
    al.refresh();
    if constexpr (!G::UNIFORM) {
#pragma unroll
      for (int i = 0; i < E; ++i) x[0][i] = src.ld(a0.v, i * a0.s);
    }
  } else {
#pragma unroll
    for (int i = 0; i < E; ++i) x[0][i] = src.ld(a0.v, i * a0.s);
  }
  xf_fwd<G, W, 1>(x, cp.xp, lds, tw, m);
#pragma unroll
  for (int i = 0; i < E; ++i) dst.st(x[0][i], al.v, i * al.s);
}

template <class W, int LOG_R, int LOG_TC, bool LZ = false>
__global__ void __launch_bounds__((ColGeo<LOG_R, LOG_TC>::THREADS))
k_colt_inv(W* out, const W* in, const W* addend, TabPtrs<W> tp, uint32_t log_n, uint32_t log_c,
           uint32_t B, uint64_t in_ls, uint64_t out_ls, int rfold, ColResc<W> rs, uint32_t aginv) {
  using G = ColGeo<LOG_R, LOG_TC>;
  constexpr int E = G::E;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  W* lds = (W*)smem_raw;
  const ColPos cp = col_pos<G>(log_c);
  const uint32_t N = 1u << log_n;
  const uint64_t ip = (uint64_t)cp.l * in_ls + (uint64_t)cp.p * N;
  const uint64_t op = (uint64_t)cp.l * out_ls + (uint64_t)cp.p * N;
  ColAddr<G, G::BB0> a0(cp, log_c);
  const ColAddr<G, G::BBL> al(cp, log_c);
  const uint32_t tl = cp.l + rs.limb0;  // this launch's limb in the basis' tables
  const LimbConst<W> lc = tp.lc[tl];
  const auto itw = col_twiddles<W, G::UNIFORM>(tp.itw + (uint64_t)tl * N, N);
  const Fold<W> f = rfold == 2 ? Fold<W>{lc.c1t, lc.c1t_p, lc.c2t, lc.c2t_p}
                  : rfold ? Fold<W>{lc.c1r, lc.c1r_p, lc.c2r, lc.c2r_p}
                          : Fold<W>{lc.c1, lc.c1_p, lc.c2, lc.c2_p};
  const BufView<W> src(in + ip, N), dst(out + op, N);
  W x[1][E];
#pragma unroll
  for (int i = 0; i < E; ++i)
    x[0][i] = src.ld(al.v, i * al.s);
  xf_inv<G, W, 1, true>(x, cp.xp, lds, itw, mod_for<W, LZ>(lc), f);  // canonical out
  a0.refresh();
  if (addend != nullptr) {
    const BufView<W> ad(addend + op, N);
    if (aginv != 0) {
      // the addend is sigma_g of the plane at `addend` (rnt_ct_rotate's
      // sigma(c0)): position pos takes its word t mod N, negated mod q when
      // t >= N, t = pos g^-1 mod 2N -- k_automorph_odd's gather (poly.rs:520-537)
#pragma unroll
      for (int i = 0; i < E; ++i) {
        const uint32_t pos = a0.v + (uint32_t)i * a0.s;
        const uint32_t t = (pos * aginv) & (2u * N - 1u);
        const W c = ad.ld(t & (N - 1u), 0u);
        x[0][i] = add_mod<W>(x[0][i], (t >= N && c != 0) ? (W)(lc.q - c) : c, lc.q);
      }
    } else {
#pragma unroll
      for (int i = 0; i < E; ++i) x[0][i] = add_mod<W>(x[0][i], ad.ld(a0.v, i * a0.s), lc.q);
    }
  }
  if (rs.last != nullptr) {
    // the fused rescale (rescale_ciphertext, engine.rs:263-282; poly.rs:187-228):
    // (c_l - (c_last mod q_l)) (q_last mod q_l)^-1, c_last the dropped
    // limb's plane of the same poly, written by this op's previous launch
    a0.refresh();
    const BufView<W> lp(rs.last + (uint64_t)cp.p * N, N);
    const W inv = rs.inv[tl], invp = rs.invp[tl];
#pragma unroll
    for (int i = 0; i < E; ++i) {
      const W cl = shoup_mul<W>(lp.ld(a0.v, i * a0.s), (W)1, lc.one_p, lc.q);
      x[0][i] = shoup_mul<W>(sub_mod<W>(x[0][i], cl, lc.q), inv, invp, lc.q);
    }
  }
  a0.refresh();
#pragma unroll
  for (int i = 0; i < E; ++i) dst.st(x[0][i], a0.v, i * a0.s);
}

// Tiled key-switch decomposition: grid x = group of jg target limbs j
// (fastest, so the workgroups that reduce one source tile of d mod every q_j
// run back to back and read it from L2; each loads the tile once and loops
// over its group), y = p * (C / TC) + column tile, z = source limb i.
template <class W, int LOG_R, int LOG_TC>
__global__ void __launch_bounds__((ColGeo<LOG_R, LOG_TC>::THREADS))
k_colt_decompose(W* __restrict__ S, const W* __restrict__ d, TabPtrs<W> tp, uint32_t log_n,
                 uint32_t log_c, uint32_t L, uint32_t B, uint64_t d_ls, uint32_t Lt,
                 uint32_t jg, uint32_t lift_csub, uint32_t skip_diag) {
  using G = ColGeo<LOG_R, LOG_TC>;
  constexpr int E = G::E;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  W* lds = (W*)smem_raw;
  const uint32_t N = 1u << log_n;
  const uint32_t tpp_log = log_c - G::LOGTC;
  const uint32_t p = blockIdx.y >> tpp_log;
  const uint32_t ct = blockIdx.y & ((1u << tpp_log) - 1);
  const uint32_t i = blockIdx.z;
  // this workgroup's target limbs: [j0, j1), the source tile loaded once
  const uint32_t j0 = blockIdx.x * jg;
  const uint32_t j1 = j0 + jg < Lt ? j0 + jg : Lt;
  ColPos cp;
  cp.xp.slot = G::slot_of(threadIdx.x);
  cp.xp.tau = G::tau_of(threadIdx.x);
  cp.xp.heap = (uint32_t)G::X;
  cp.col = (ct << G::LOGTC) + cp.xp.slot;
  const ColAddr<G, G::BB0> a0(cp, log_c);
  ColAddr<G, G::BBL> al(cp, log_c);
  const BufView<W> src(d + (uint64_t)i * d_ls + (uint64_t)p * N, N);
  W raw[E];
#pragma unroll
  for (int e = 0; e < E; ++e) raw[e] = src.ld(a0.v, e * a0.s);
#pragma unroll 1
  for (uint32_t j = j0; j < j1; ++j) {
    // the diagonal (target j == source i) is the tensor's own d2^ (k_ks_rows
    // reads it there): no transform, no S plane
    if (skip_diag && j == i) continue;
    const BufView<W> dst(S + (((uint64_t)j * L + i) * B + p) * N, N);
    const LimbConst<W> lc = tp.lc[j];
    W x[1][E];
    // alpha_i mod q_j: one conditional subtraction when every word is below
    // 2 q_j (u32 words, all target q_j > 2^30), else a Shoup reduction
    if (lift_csub) {
#pragma unroll
      for (int e = 0; e < E; ++e) x[0][e] = csub<W>(raw[e], lc.q);
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e) x[0][e] = shoup_mul<W>(raw[e], (W)1, lc.one_p, lc.q);
    }
    // (the transform's LDS exchange ends in a barrier: the next j may reuse it)
    xf_fwd<G, W, 1>(x, cp.xp, lds, col_twiddles<W, G::UNIFORM>(tp.tw + (uint64_t)j * N, N),
                    mod_of(lc));
    al.refresh();
#pragma unroll
    for (int e = 0; e < E; ++e) dst.st(x[0][e], al.v, e * al.s);
  }
}

#define RNT_DISPATCH_LOGR(LOGR, MACRO) \
  switch (LOGR) {                      \
    case 0: MACRO(0); break;           \
    case 1: MACRO(1); break;           \
    case 2: MACRO(2); break;           \
    case 3: MACRO(3); break;           \
    case 4: MACRO(4); break;           \
    default: return hipErrorInvalidValue; \
  }

#define RNT_DISPATCH_LOGRT(LOGR, MACRO) \
  switch (LOGR) {                       \
    case 5: MACRO(5); break;            \
    case 6: MACRO(6); break;            \
    case 7: MACRO(7); break;            \
    case 8: MACRO(8); break;            \
    default: return hipErrorInvalidValue; \
  }

template <class W, int LOG_R, int LOG_TC>
static size_t col_lds() {
  return (size_t)ColGeo<LOG_R, LOG_TC>::REGION * sizeof(W);
}

// Tiled column grid: x = poly * (C / TC) + column tile, y, z as given
// (limb; source x target limb for the key-switch decomposition).  grid.x = 0
// flags a shape beyond the hardware grid limits.
static int col_log_tc(const Geom& g) { return g.log_c >= 6 ? 6 : 5; }
static dim3 col_grid(const Launch& k, const Geom& g, uint32_t y, uint32_t z) {
  const uint64_t x = (uint64_t)k.B << (g.log_c - col_log_tc(g));
  if (x > 0x7fffffffull || y > 65535u || z > 65535u) return dim3(0, 1, 1);
  return dim3((unsigned)x, y, z);
}

template <class W, bool LZ>
static hipError_t col_fwd_t(const Launch& k, void* out0, const void* in0, void* out1,
                            const void* in1, uint64_t in_ls, uint64_t out_ls) {
  const Geom g = geom_for(k.t->log_n);
  const TabPtrs<W> tp = tab_ptrs<W>(k.t, k.tab0);
  if ((uint64_t)k.L * k.B == 0) return hipSuccess;
  if (g.log_r >= 5) {
    const dim3 grid = col_grid(k, g, (uint32_t)k.L, 1);
    if (grid.x == 0) return hipErrorInvalidConfiguration;
    hipError_t e = hipSuccess;
#define RNT_L2(R, TC)                                                                           \
  e = allow_lds(k_colt_fwd<W, R, TC, LZ>, col_lds<W, R, TC>());                                 \
  if (e != hipSuccess) return e;                                                                \
  hipLaunchKernelGGL((k_colt_fwd<W, R, TC, LZ>), grid, dim3(ColGeo<R, TC>::THREADS),                \
                     (col_lds<W, R, TC>()), k.s, (W*)out0, (const W*)in0, (W*)out1, (const W*)in1, \
                     tp, g.log_n, g.log_c, (uint32_t)k.B, in_ls, out_ls)
#define RNT_L(R)                          \
  if (col_log_tc(g) == 6) {               \
    RNT_L2(R, 6);                         \
  } else {                                \
    RNT_L2(R, 5);                         \
  }
    RNT_DISPATCH_LOGRT(g.log_r, RNT_L)
#undef RNT_L
#undef RNT_L2
    return hipGetLastError();
  }
  const uint64_t total = (uint64_t)k.L * k.B * g.c;
#define RNT_L(R)                                                                              \
  hipLaunchKernelGGL((k_col_fwd<W, R>), dim3(grid_for(total, 256)), dim3(256), 0, k.s,      \
                     (W*)out0, (const W*)in0, (W*)out1, (const W*)in1, tp, g.log_n, g.log_c, \
                     (uint32_t)k.B, in_ls, out_ls, total)
  RNT_DISPATCH_LOGR(g.log_r, RNT_L)
#undef RNT_L
  return hipGetLastError();
}

template <class W, bool LZ>
static hipError_t col_inv_t(const Launch& k, void* out, uint64_t out_ls, const void* in,
                            uint64_t in_ls, int rfold, const void* addend, const ColRescArgs& ra) {
  ColResc<W> rs;
  rs.last = (const W*)ra.last;
  rs.inv = (const W*)ra.inv;
  rs.invp = (const W*)ra.invp;
  rs.limb0 = ra.limb0;
  const Geom g = geom_for(k.t->log_n);
  const TabPtrs<W> tp = tab_ptrs<W>(k.t, k.tab0);
  if ((uint64_t)k.L * k.B == 0) return hipSuccess;
  if (g.log_r >= 5) {
    const dim3 grid = col_grid(k, g, (uint32_t)k.L, 1);
    if (grid.x == 0) return hipErrorInvalidConfiguration;
    hipError_t e = hipSuccess;
#define RNT_L2(R, TC)                                                                        \
  e = allow_lds(k_colt_inv<W, R, TC, LZ>, col_lds<W, R, TC>());                              \
  if (e != hipSuccess) return e;                                                             \
  hipLaunchKernelGGL((k_colt_inv<W, R, TC, LZ>), grid, dim3(ColGeo<R, TC>::THREADS),             \
                     (col_lds<W, R, TC>()), k.s, (W*)out, (const W*)in, (const W*)addend, tp, \
                     g.log_n, g.log_c, (uint32_t)k.B, in_ls, out_ls, rfold, rs, k.add_ginv)
#define RNT_L(R)                          \
  if (col_log_tc(g) == 6) {               \
    RNT_L2(R, 6);                         \
  } else {                                \
    RNT_L2(R, 5);                         \
  }
    RNT_DISPATCH_LOGRT(g.log_r, RNT_L)
#undef RNT_L
#undef RNT_L2
    return hipGetLastError();
  }
  if (ra.last != nullptr || ra.limb0 != 0 || (addend != nullptr && k.add_ginv != 0))
    return hipErrorInvalidValue;  // tiled grids only (log R >= 5)
  const uint64_t total = (uint64_t)k.L * k.B * g.c;
#define RNT_L(R)                                                                          \
  hipLaunchKernelGGL((k_col_inv<W, R>), dim3(grid_for(total, 256)), dim3(256), 0, k.s,  \
                     (W*)out, (const W*)in, (const W*)addend, tp, g.log_n, g.log_c,      \
                     (uint32_t)k.B, in_ls, out_ls, total, rfold)
  RNT_DISPATCH_LOGR(g.log_r, RNT_L)
#undef RNT_L
  return hipGetLastError();
}

template <class W>
static hipError_t ks_decompose_t(const Launch& k, void* S, const void* d, uint64_t d_ls) {
  const Geom g = geom_for(k.t->log_n);
  if ((uint64_t)k.L * k.B == 0) return hipSuccess;
  const TabPtrs<W> tp = tab_ptrs<W>(k.t);
  const uint32_t Ls = (uint32_t)k.src_limbs();  // source limbs i; target limbs j = k.L
  if (g.log_r >= 5) {
    const dim3 g0 = col_grid(k, g, Ls, (uint32_t)k.L);
    if (g0.x == 0 || g0.x > 65535u) return hipErrorInvalidConfiguration;
    // target limbs per workgroup (Tables::dec_jg; 0 = auto): the source tile
    // is read once per group instead of once per target limb.  Auto takes
    // groups of 16 (vs one limb per group: ks_decompose -8%, profiles/r01_ab_dec_jg.txt) and
    // halves them while the grid would fall under 4 workgroups per CU.
    uint32_t jg = k.t->dec_jg;
    if (jg == 0) {
      jg = 16;
      while (jg > 1 && ((uint32_t)k.L + jg - 1) / jg * (uint64_t)g0.x * Ls < 1024u) jg >>= 1;
    }
    const dim3 grid(((uint32_t)k.L + jg - 1) / jg, g0.x, Ls);
    // u32 words hold residues of moduli < 2^31 (wider bases take u64), so
    // alpha_i < 2^31 <= 2 q_j when every target modulus is >= 2^30: one
    // conditional subtraction reduces it (the root basis' smallest modulus
    // bounds every drop_last view's)
    uint64_t qmin = ~0ull;
    for (uint64_t q : k.t->moduli) qmin = q < qmin ? q : qmin;
    const uint32_t lift_csub = sizeof(W) == 4 && qmin >= (1ull << 30) ? 1u : 0u;
    if (k.d2hat != nullptr && Ls != (uint32_t)k.L) return hipErrorInvalidValue;  // the diagonal needs one basis
    const uint32_t skip_diag = k.d2hat != nullptr ? 1u : 0u;
    hipError_t e = hipSuccess;
#define RNT_L2(R, TC)                                                                         \
  e = allow_lds(k_colt_decompose<W, R, TC>, col_lds<W, R, TC>());                             \
  if (e != hipSuccess) return e;                                                              \
  hipLaunchKernelGGL((k_colt_decompose<W, R, TC>), grid, dim3(ColGeo<R, TC>::THREADS),        \
                     (col_lds<W, R, TC>()), k.s, (W*)S, (const W*)d, tp, g.log_n, g.log_c,      \
                     Ls, (uint32_t)k.B, d_ls, (uint32_t)k.L, jg, lift_csub, skip_diag)
#define RNT_L(R)                          \
  if (col_log_tc(g) == 6) {               \
    RNT_L2(R, 6);                         \
  } else {                                \
    RNT_L2(R, 5);                         \
  }
    RNT_DISPATCH_LOGRT(g.log_r, RNT_L)
#undef RNT_L
#undef RNT_L2
    return hipGetLastError();
  }
  if (k.d2hat != nullptr) return hipErrorInvalidValue;  // the diagonal skip: tiled grids only
  const uint64_t total = (uint64_t)k.L * Ls * k.B * g.c;
#define RNT_L(R)                                                                               \
  hipLaunchKernelGGL((k_ks_decompose<W, R>), dim3(grid_for(total, 256)), dim3(256), 0, k.s,  \
                     (W*)S, (const W*)d, tp, g.log_n, g.log_c, Ls, (uint32_t)k.B, d_ls, total)
  RNT_DISPATCH_LOGR(g.log_r, RNT_L)
#undef RNT_L
  return hipGetLastError();
}

// The Harvey-lazy product path: u32 words with every q < 2^30 (lazy30) or
// u64 words with every q < 2^62 (lazy62), on the tiled column grids.
bool lazy_ok(const Tables* t) {
  return (t->wide ? t->lazy62 : t->lazy30) && geom_for(t->log_n).log_r >= 5;
}
hipError_t launch_col_fwd(const Launch& k, void* out0, const void* in0, void* out1,
                          const void* in1, uint64_t in_ls, uint64_t out_ls, bool lazy) {
  const bool lz = lazy && lazy_ok(k.t);
  if (k.t->wide)
    return lz ? col_fwd_t<uint64_t, true>(k, out0, in0, out1, in1, in_ls, out_ls)
              : col_fwd_t<uint64_t, false>(k, out0, in0, out1, in1, in_ls, out_ls);
  return lz ? col_fwd_t<uint32_t, true>(k, out0, in0, out1, in1, in_ls, out_ls)
            : col_fwd_t<uint32_t, false>(k, out0, in0, out1, in1, in_ls, out_ls);
}

hipError_t launch_col_inv(const Launch& k, void* out, uint64_t out_ls, const void* in,
                          uint64_t in_ls, int rfold, const void* addend, bool lazy, const ColRescArgs& ra) {
  const bool lz = lazy && lazy_ok(k.t);
  if (k.t->wide)
    return lz ? col_inv_t<uint64_t, true>(k, out, out_ls, in, in_ls, rfold, addend, ra)
              : col_inv_t<uint64_t, false>(k, out, out_ls, in, in_ls, rfold, addend, ra);
  return lz ? col_inv_t<uint32_t, true>(k, out, out_ls, in, in_ls, rfold, addend, ra)
            : col_inv_t<uint32_t, false>(k, out, out_ls, in, in_ls, rfold, addend, ra);
}
bool col_resc_ok(const Tables* t) { return geom_for(t->log_n).log_r >= 5; }
const void* resc_inv_row(const Tables* t, size_t last, int which) {
  const size_t wb = t->wide ? 8 : 4;
  const char* base = (const char*)(which ? t->resc_p : t->resc);
  return base + last * t->L * wb;
}

hipError_t launch_ks_decompose(const Launch& k, void* S, const void* d, uint64_t d_ls) {
  return by_word(k, [&](auto w) { return ks_decompose_t<decltype(w)>(k, S, d, d_ls); });
}
}  // namespace rnt
