// rnt_kernels.hip -- the streaming gfx950 kernels of the RNS-NTT hot path and
// their launchers: elementwise, broadcast / BSGS / hoisted MACs, ModUp,
// ModDown*, lincomb, dot_tensor, plain_mac, rescale, automorphism, import /
// export, copy, CRT.  The four-step transform lives in rnt_col.hip (column
// passes) and rnt_rows.hip (row passes, key-switch rows, tensor rows) over
// rnt_fourstep.hpp.
//
// Reference behaviour being replaced (oiwn/toy-heaan-ckks):
//   MulAssign (NTT domain)            src/rings/backends/rns_ntt/poly.rs:277-331
//   AddAssign / Neg                   poly.rs:254-275, 370-385
//   rescale_into                      poly.rs:187-228
//   automorphism                      poly.rs:492-541
#include <hip/hip_runtime.h>

#include "rnt_device.hpp"
#include "rnt_internal.hpp"
#include "rnt_launch.hpp"
#include "rnt_modarith.hpp"

namespace rnt {

// ---------------------------------------------------------------------------
// elementwise / permutation kernels
// ---------------------------------------------------------------------------

template <class W, int OP>
__device__ __forceinline__ W elementwise_op(W x, W y, const LimbConst<W>& lc) {
  if constexpr (OP == 0) return add_mod<W>(x, y, lc.q);
  else if constexpr (OP == 1) return sub_mod<W>(x, y, lc.q);
  else if constexpr (OP == 2) return x == 0 ? (W)0 : (W)(lc.q - x);
  else if constexpr (OP == 3) return shoup_mul<W>(mont_mul<W>(x, y, lc.q, lc.qinv), lc.rmod, lc.rmod_p, lc.q);
  else return mont_mul<W>(x, y, lc.q, lc.qinv);
}

// Coefficient-wise ops (poly.rs:254-306, 370-385).  Grid: x = chunks of one
// limb's B*N words, y = limb, so the limb constants are wave-uniform (no
// per-thread division).  VEC: every thread moves 16 bytes per operand
// (callers check 16-byte alignment and a limb length divisible by it).
template <class W, int OP, bool VEC>
__global__ void __launch_bounds__(256)
k_elementwise(W* __restrict__ out, const W* __restrict__ a, const W* __restrict__ b,
              TabPtrs<W> tp, uint64_t limb_words) {
  constexpr int V = VEC ? 16 / (int)sizeof(W) : 1;
  const uint32_t l = blockIdx.y;
  const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (i >= limb_words) return;
  const LimbConst<W> lc = tp.lc[l];
  const uint64_t g = (uint64_t)l * limb_words + i;
  if constexpr (VEC) {
    const uint4 xa = *reinterpret_cast<const uint4*>(a + g);
    uint4 xb = xa;
    if constexpr (OP != 2) xb = *reinterpret_cast<const uint4*>(b + g);
    W x[V], y[V], r[V];
    __builtin_memcpy(x, &xa, 16);
    __builtin_memcpy(y, &xb, 16);
#pragma unroll
    for (int v = 0; v < V; ++v) r[v] = elementwise_op<W, OP>(x[v], y[v], lc);
    uint4 o;
    __builtin_memcpy(&o, r, 16);
    *reinterpret_cast<uint4*>(out + g) = o;
  } else {
    out[g] = elementwise_op<W, OP>(a[g], OP == 2 ? (W)0 : b[g], lc);
  }
}

// Pointwise products of rnt_ct_linear over a batch [L][B][N] (limb stride B N
// words), grid as k_elementwise.  KIND 0: out = x (.) m 2^-w (Montgomery
// product) with m one plane per limb (limb stride m_ls, the same plane for
// every poly of the batch), or x 2^-w where m is null (the key-switch seed
// scale); with `accum` (uniform) the product is added to out.  KIND 1:
// out = x 2^w mod q (a canonical plaintext into Montgomery form, so that a
// later Montgomery product with it is the canonical product).  out may be x.
template <class W, int KIND, bool VEC>
__global__ void __launch_bounds__(256)
k_bcast_mul(W* out, const W* x, const W* __restrict__ m, TabPtrs<W> tp, uint32_t log_n,
            uint64_t limb_words, uint64_t m_ls, uint32_t accum) {
  constexpr int V = VEC ? 16 / (int)sizeof(W) : 1;
  const uint32_t l = blockIdx.y;
  const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (i >= limb_words) return;
  const LimbConst<W> lc = tp.lc[l];
  const uint64_t g = (uint64_t)l * limb_words + i;
  const uint64_t mi = (uint64_t)l * m_ls + (i & ((1ull << log_n) - 1));  // V divides N: one plane
  W xv[V], mv[V], ov[V], r[V];
  if constexpr (VEC) {
    const uint4 xa = *reinterpret_cast<const uint4*>(x + g);
    __builtin_memcpy(xv, &xa, 16);
  } else {
    xv[0] = x[g];
  }
#pragma unroll
  for (int v = 0; v < V; ++v) mv[v] = (W)1;
  if (KIND == 0 && m != nullptr) {
    if constexpr (VEC) {
      const uint4 ma = *reinterpret_cast<const uint4*>(m + mi);
      __builtin_memcpy(mv, &ma, 16);
    } else {
      mv[0] = m[mi];
    }
  }
#pragma unroll
  for (int v = 0; v < V; ++v) {
    if constexpr (KIND == 0) r[v] = mont_mul<W>(xv[v], mv[v], lc.q, lc.qinv);
    else r[v] = shoup_mul<W>(xv[v], lc.rmod, lc.rmod_p, lc.q);
  }
  if (KIND == 0 && accum) {
    if constexpr (VEC) {
      const uint4 oa = *reinterpret_cast<const uint4*>(out + g);
      __builtin_memcpy(ov, &oa, 16);
    } else {
      ov[0] = out[g];
    }
#pragma unroll
    for (int v = 0; v < V; ++v) r[v] = add_mod<W>(ov[v], r[v], lc.q);
  }
  if constexpr (VEC) {
    uint4 o;
    __builtin_memcpy(&o, r, 16);
    *reinterpret_cast<uint4*>(out + g) = o;
  } else {
    out[g] = r[0];
  }
}

// The inner sums of rnt_ct_linear_bsgs in the NTT domain, both components of
// up to BSGS_JT giant steps per launch: out_jj = sum_b x_b (.) m[jj][b] for
// jj < nj.  x is the baby rotations, block 2 b + comp of blk_words words
// ([L][B][N], limb stride B N) for blockIdx.z = comp; m points at plane
// (jj = 0, b = 0) of the Montgomery-form plaintexts ([L][..][N] at limb stride
// m_ls, plane jj n_baby + b, the same plane for every poly of the batch), so
// every Montgomery product is the canonical product and the sums stay
// canonical through add_mod.  Output jj is o.out[jj] + comp blk_words; with
// bit jj of accum_mask the sum is added to the words already there.  A thread
// reads each baby vector once for all nj sums: 2 n_baby + 2 nj batch-planes
// of traffic per launch against the 6 n_baby nj of one k_bcast_mul per pair.
constexpr int BSGS_JT = (int)kBsgsJt;
template <class W>
struct BsgsOuts {
  W* out[BSGS_JT];
};
template <class W, bool VEC>
__global__ void __launch_bounds__(256)
k_bsgs_mac(BsgsOuts<W> o, const W* __restrict__ x, const W* __restrict__ m, TabPtrs<W> tp, uint32_t log_n,
           uint64_t limb_words, uint64_t blk_words, uint64_t m_ls, uint32_t n_baby, uint32_t nj,
           uint32_t accum_mask) {
  constexpr int V = VEC ? 16 / (int)sizeof(W) : 1;
  const uint32_t l = blockIdx.y;
  const uint32_t comp = blockIdx.z;
  const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (i >= limb_words) return;
  const LimbConst<W> lc = tp.lc[l];
  const uint64_t N = 1ull << log_n;
  const uint64_t g = (uint64_t)comp * blk_words + (uint64_t)l * limb_words + i;
  const W* mp = m + (uint64_t)l * m_ls + (i & (N - 1));  // V divides N: one plane
  const W* xp = x + g;
  W acc[BSGS_JT][V];
#pragma unroll
  for (int jj = 0; jj < BSGS_JT; ++jj)
#pragma unroll
    for (int v = 0; v < V; ++v) acc[jj][v] = (W)0;
  for (uint32_t b = 0; b < n_baby; ++b) {
    W xv[V];
    if constexpr (VEC) {
      const uint4 xa = *reinterpret_cast<const uint4*>(xp + (uint64_t)b * 2 * blk_words);
      __builtin_memcpy(xv, &xa, 16);
    } else {
      xv[0] = xp[(uint64_t)b * 2 * blk_words];
    }
#pragma unroll
    for (int jj = 0; jj < BSGS_JT; ++jj) {
      if ((uint32_t)jj < nj) {  // (uniform)
        const W* mq = mp + ((uint64_t)jj * n_baby + b) * N;
        W mv[V];
        if constexpr (VEC) {
          const uint4 ma = *reinterpret_cast<const uint4*>(mq);
          __builtin_memcpy(mv, &ma, 16);
        } else {
          mv[0] = mq[0];
        }
#pragma unroll
        for (int v = 0; v < V; ++v)
          acc[jj][v] = add_mod<W>(acc[jj][v], mont_mul<W>(xv[v], mv[v], lc.q, lc.qinv), lc.q);
      }
    }
  }
#pragma unroll
  for (int jj = 0; jj < BSGS_JT; ++jj) {
    if ((uint32_t)jj < nj) {
      W* op = o.out[jj] + g;
      if ((accum_mask >> jj) & 1u) {
        W ov[V];
        if constexpr (VEC) {
          const uint4 oa = *reinterpret_cast<const uint4*>(op);
          __builtin_memcpy(ov, &oa, 16);
        } else {
          ov[0] = op[0];
        }
#pragma unroll
        for (int v = 0; v < V; ++v) acc[jj][v] = add_mod<W>(ov[v], acc[jj][v], lc.q);
      }
      if constexpr (VEC) {
        uint4 r;
        __builtin_memcpy(&r, acc[jj], 16);
        *reinterpret_cast<uint4*>(op) = r;
      } else {
        op[0] = acc[jj][0];
      }
    }
  }
}

// One [N] plane per limb of Montgomery ones (2^w mod q): the plaintext row of
// the LIN key-switch rows where a term has no plaintext (the giant rotations
// of rnt_ct_linear_bsgs).
template <class W>
__global__ void __launch_bounds__(256)
k_mont_one(W* __restrict__ out, TabPtrs<W> tp, uint32_t log_n) {
  const uint32_t l = blockIdx.y;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (1u << log_n)) return;
  out[((uint64_t)l << log_n) + i] = tp.lc[l].rmod;
}

// The gadget digits of the hoisted rotations before their forward transform:
// D[j][i][p] = (c1 limb i, poly p) 2^w mod q_j, canonical, for every target
// limb j < L.  Grid (16-byte vectors of a source limb's chunk, source limb i);
// a thread reads its source vector once and writes the L residues.  c1 is the
// chunk's first poly at limb stride src_ls; D is [L][gridDim.y][B][N].  The
// factor 2^w (Montgomery form, linear through the transform) is what makes
// k_hoist_mac's Montgomery products with the canonical keys canonical.
template <class W, bool VEC>
__global__ void __launch_bounds__(256)
k_hoist_digits(W* __restrict__ D, const W* __restrict__ c1, TabPtrs<W> tp, uint64_t limb_words,
               uint64_t src_ls, uint32_t L) {
  constexpr int V = VEC ? 16 / (int)sizeof(W) : 1;
  const uint32_t s = blockIdx.y;
  const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (i >= limb_words) return;
  W xv[V];
  if constexpr (VEC) {
    const uint4 xa = *reinterpret_cast<const uint4*>(c1 + (uint64_t)s * src_ls + i);
    __builtin_memcpy(xv, &xa, 16);
  } else {
    xv[0] = c1[(uint64_t)s * src_ls + i];
  }
  for (uint32_t j = 0; j < L; ++j) {
    const LimbConst<W> lc = tp.lc[j];
    W* dp = D + ((uint64_t)j * gridDim.y + s) * limb_words + i;
    W r[V];
#pragma unroll
    for (int v = 0; v < V; ++v) r[v] = shoup_mul<W>(xv[v], lc.rmod, lc.rmod_p, lc.q);
    if constexpr (VEC) {
      uint4 o;
      __builtin_memcpy(&o, r, 16);
      *reinterpret_cast<uint4*>(dp) = o;
    } else {
      dp[0] = r[0];
    }
  }
}

// The gadget sums of up to HOIST_T hoisted rotations of one chunk in the NTT
// domain: acc0[t] = sum_i D^[j][i] (.) key_b[t][i], acc1[t] with key_a, for
// t < nt.  d is the transformed Montgomery-form digits ([L][Ls][B][N]); the
// keys are in hoisting form, key_*[t] pointing at (source limb 0, limb 0) of
// step t's key: source limb i at + i N, limb j at + j key_ls, the same plane
// for every poly of the batch.  Grid (16-byte vectors of a target limb's
// chunk, target limb j); a thread holds one vector position, loops over the Ls
// source limbs, reads each digit vector once and keeps 2 HOIST_T accumulators.
// mont_mul(d 2^w, key) is the canonical product and the sums stay canonical
// through add_mod.  No gather: the pre-rotated keys make it a stream.
constexpr int HOIST_T = (int)kHoistT;

template <class W>
struct HoistArgs {
  const W* key_b[HOIST_T];
  const W* key_a[HOIST_T];
  W* acc0[HOIST_T];
  W* acc1[HOIST_T];
};
template <class W, bool VEC>
__global__ void __launch_bounds__(256)
k_hoist_mac(HoistArgs<W> a, const W* __restrict__ d, TabPtrs<W> tp, uint32_t log_n, uint64_t limb_words,
            uint64_t key_ls, uint32_t Ls, uint32_t nt, LimbMap lm) {
  constexpr int V = VEC ? 16 / (int)sizeof(W) : 1;
  const uint32_t j = blockIdx.y;
  const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (i >= limb_words) return;
  const uint32_t rj = root_limb(j, lm);
  const LimbConst<W> lc = tp.lc[rj];
  const uint64_t N = 1ull << log_n;
  const W* dp = d + (uint64_t)j * Ls * limb_words + i;
  const uint64_t ko = (uint64_t)rj * key_ls + (i & (N - 1));  // V divides N: one plane
  W acc0[HOIST_T][V], acc1[HOIST_T][V];
#pragma unroll
  for (int t = 0; t < HOIST_T; ++t)
#pragma unroll
    for (int v = 0; v < V; ++v) acc0[t][v] = acc1[t][v] = (W)0;
  for (uint32_t s = 0; s < Ls; ++s) {
    W xv[V];
    if constexpr (VEC) {
      const uint4 xa = *reinterpret_cast<const uint4*>(dp + (uint64_t)s * limb_words);
      __builtin_memcpy(xv, &xa, 16);
    } else {
      xv[0] = dp[(uint64_t)s * limb_words];
    }
#pragma unroll
    for (int t = 0; t < HOIST_T; ++t) {
      if ((uint32_t)t < nt) {  // (uniform)
        const W* bq = a.key_b[t] + ko + (uint64_t)s * N;
        const W* aq = a.key_a[t] + ko + (uint64_t)s * N;
        W bv[V], av[V];
        if constexpr (VEC) {
          const uint4 b4 = *reinterpret_cast<const uint4*>(bq);
          const uint4 a4 = *reinterpret_cast<const uint4*>(aq);
          __builtin_memcpy(bv, &b4, 16);
          __builtin_memcpy(av, &a4, 16);
        } else {
          bv[0] = bq[0];
          av[0] = aq[0];
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
          acc0[t][v] = add_mod<W>(acc0[t][v], mont_mul<W>(xv[v], bv[v], lc.q, lc.qinv), lc.q);
          acc1[t][v] = add_mod<W>(acc1[t][v], mont_mul<W>(xv[v], av[v], lc.q, lc.qinv), lc.q);
        }
      }
    }
  }
  const uint64_t g = (uint64_t)j * limb_words + i;
#pragma unroll
  for (int t = 0; t < HOIST_T; ++t) {
    if ((uint32_t)t < nt) {
      if constexpr (VEC) {
        uint4 r0, r1;
        __builtin_memcpy(&r0, acc0[t], 16);
        __builtin_memcpy(&r1, acc1[t], 16);
        *reinterpret_cast<uint4*>(a.acc0[t] + g) = r0;
        *reinterpret_cast<uint4*>(a.acc1[t] + g) = r1;
      } else {
        a.acc0[t][g] = acc0[t][0];
        a.acc1[t][g] = acc1[t][0];
      }
    }
  }
}

// k_hoist_mac with the sums ADDED to what acc0[t] / acc1[t] hold (canonical):
// the giant stage of rnt_ct_linear_bsgs_hybrid, whose one A0, A1 are summed over
// several launches.  A kernel of its own, so that k_hoist_mac stays as it is.
template <class W, bool VEC>
__global__ void __launch_bounds__(256)
k_hoist_mac_acc(HoistArgs<W> a, const W* __restrict__ d, TabPtrs<W> tp, uint32_t log_n, uint64_t limb_words,
                uint64_t key_ls, uint32_t Ls, uint32_t nt, LimbMap lm) {
  constexpr int V = VEC ? 16 / (int)sizeof(W) : 1;
  const uint32_t j = blockIdx.y;
  const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (i >= limb_words) return;
  const uint32_t rj = root_limb(j, lm);
  const LimbConst<W> lc = tp.lc[rj];
  const uint64_t N = 1ull << log_n;
  const W* dp = d + (uint64_t)j * Ls * limb_words + i;
  const uint64_t ko = (uint64_t)rj * key_ls + (i & (N - 1));  // V divides N: one plane
  const uint64_t g = (uint64_t)j * limb_words + i;
  W acc0[HOIST_T][V], acc1[HOIST_T][V];
#pragma unroll
  for (int t = 0; t < HOIST_T; ++t) {
#pragma unroll
    for (int v = 0; v < V; ++v) acc0[t][v] = acc1[t][v] = (W)0;
    if ((uint32_t)t < nt) {  // (uniform)
      if constexpr (VEC) {
        const uint4 r0 = *reinterpret_cast<const uint4*>(a.acc0[t] + g);
        const uint4 r1 = *reinterpret_cast<const uint4*>(a.acc1[t] + g);
        __builtin_memcpy(acc0[t], &r0, 16);
        __builtin_memcpy(acc1[t], &r1, 16);
      } else {
        acc0[t][0] = a.acc0[t][g];
        acc1[t][0] = a.acc1[t][g];
      }
    }
  }
  for (uint32_t s = 0; s < Ls; ++s) {
    W xv[V];
    if constexpr (VEC) {
      const uint4 xa = *reinterpret_cast<const uint4*>(dp + (uint64_t)s * limb_words);
      __builtin_memcpy(xv, &xa, 16);
    } else {
      xv[0] = dp[(uint64_t)s * limb_words];
    }
#pragma unroll
    for (int t = 0; t < HOIST_T; ++t) {
      if ((uint32_t)t < nt) {  // (uniform)
        const W* bq = a.key_b[t] + ko + (uint64_t)s * N;
        const W* aq = a.key_a[t] + ko + (uint64_t)s * N;
        W bv[V], av[V];
        if constexpr (VEC) {
          const uint4 b4 = *reinterpret_cast<const uint4*>(bq);
          const uint4 a4 = *reinterpret_cast<const uint4*>(aq);
          __builtin_memcpy(bv, &b4, 16);
          __builtin_memcpy(av, &a4, 16);
        } else {
          bv[0] = bq[0];
          av[0] = aq[0];
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
          acc0[t][v] = add_mod<W>(acc0[t][v], mont_mul<W>(xv[v], bv[v], lc.q, lc.qinv), lc.q);
          acc1[t][v] = add_mod<W>(acc1[t][v], mont_mul<W>(xv[v], av[v], lc.q, lc.qinv), lc.q);
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < HOIST_T; ++t) {
    if ((uint32_t)t < nt) {
      if constexpr (VEC) {
        uint4 r0, r1;
        __builtin_memcpy(&r0, acc0[t], 16);
        __builtin_memcpy(&r1, acc1[t], 16);
        *reinterpret_cast<uint4*>(a.acc0[t] + g) = r0;
        *reinterpret_cast<uint4*>(a.acc1[t] + g) = r1;
      } else {
        a.acc0[t][g] = acc0[t][0];
        a.acc1[t][g] = acc1[t][0];
      }
    }
  }
}

// The automorphism sigma_g (g odd) in the NTT domain is a pure permutation of
// evaluation points, with no sign: sigma_g(a)(psi^(2k+1)) = a(psi^(g (2k+1))),
// and the device holds device[brv(k)] = a(psi^(2k+1)) (rnt_internal.hpp).  So
// position p of the output reads position
//   brv(((g (2 brv(p) + 1) mod 2N) - 1) / 2)
// of the input.  The map is a bijection and BLOCK-STRUCTURED: for every m an
// aligned block of 2^m positions reads from one aligned block of 2^m positions
// (the top log_n - m bits of p are the low bits of k, and g (2k + 1) mod
// 2^(log_n - m + 1) depends on those alone), permuted inside.  A wave of 64
// lanes x 16 bytes therefore gathers from exactly one aligned span of its own
// size: word-granular loads, but every cache line fetched is used whole.
// tests/test_rotsum_ref.py pins both properties.  g < 2N <= 2^18; the product
// wraps mod 2^32, a multiple of 2N.
__device__ __forceinline__ uint32_t ntt_automorph_src(uint32_t p, uint32_t g, uint32_t log_n) {
  const uint32_t sh = 32u - log_n;
  const uint32_t k = __brev(p) >> sh;
  const uint32_t e = (g * (2u * k + 1u)) & ((2u << log_n) - 1u);
  return __brev(e >> 1) >> sh;
}

// out = the NTT-domain words of sigma_g(in), in in the NTT domain (g odd): the
// gather above within every plane.  Grid as k_elementwise (x = the words of a
// limb's chunk, y = limb), one word per thread.
template <class W>
__global__ void __launch_bounds__(256)
k_automorph_ntt(W* __restrict__ out, const W* __restrict__ in, uint32_t log_n, uint32_t g, uint64_t limb_words) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= limb_words) return;
  const uint64_t N = 1ull << log_n;
  const uint64_t base = (uint64_t)blockIdx.y * limb_words + (i & ~(N - 1));
  out[base + (i & (N - 1))] = in[base + ntt_automorph_src((uint32_t)(i & (N - 1)), g, log_n)];
}

// The key products of a rotate-and-sum (rnt_ct_rotsum_hybrid) for up to
// ROTSUM_T steps of one chunk in the NTT domain:
//   acc0 (+)= sum_{t < nt} sum_s sigma_{g_t}(D^[j][s]) (.) key_b[t][s],  acc1 with key_a.
// d is the transformed Montgomery-form digits ([L][Ls][B][N], hybrid_raise);
// the keys are ORDINARY prepared keys, key_*[t] pointing at (digit 0, limb 0)
// of step t's key: digit s at + s N, limb j at + j key_ls, the same plane for
// every poly of the batch.  Grid as k_hoist_mac; a thread owns one vector
// position and the two accumulators.  Per step it computes its V source
// positions once (ntt_automorph_src), then per digit gathers the V digit words
// at them inside the poly's own plane, streams the two key vectors and adds the
// Montgomery products -- canonical, as in k_hoist_mac.  The steps run in a loop
// over the table in the kernel arguments, so the registers do not grow with
// ROTSUM_T.  ACC: the sums start from what acc0 / acc1 hold (the groups after
// the first).
constexpr int ROTSUM_T = (int)kRotsumT;

template <class W>
struct RotsumArgs {
  const W* key_b[ROTSUM_T];
  const W* key_a[ROTSUM_T];
  uint32_t g[ROTSUM_T];
};
template <class W, bool VEC, bool ACC>
__global__ void __launch_bounds__(256)
k_rotsum_mac(W* acc0, W* acc1, RotsumArgs<W> a, const W* __restrict__ d, TabPtrs<W> tp, uint32_t log_n,
             uint64_t limb_words, uint64_t key_ls, uint32_t Ls, uint32_t nt, LimbMap lm) {
  constexpr int V = VEC ? 16 / (int)sizeof(W) : 1;
  const uint32_t j = blockIdx.y;
  const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (i >= limb_words) return;
  const uint32_t rj = root_limb(j, lm);
  const LimbConst<W> lc = tp.lc[rj];
  const uint64_t N = 1ull << log_n;
  const uint32_t p0 = (uint32_t)(i & (N - 1));  // V divides N: one plane
  const W* dp = d + (uint64_t)j * Ls * limb_words + (i - p0);
  const uint64_t ko = (uint64_t)rj * key_ls + p0;
  const uint64_t o = (uint64_t)j * limb_words + i;
  W s0[V], s1[V];
  if constexpr (ACC) {
    ld_vec<W, VEC, V>(s0, acc0 + o);
    ld_vec<W, VEC, V>(s1, acc1 + o);
  } else {
#pragma unroll
    for (int v = 0; v < V; ++v) s0[v] = s1[v] = (W)0;
  }
  for (uint32_t t = 0; t < nt; ++t) {  // (uniform)
    const uint32_t g = a.g[t];
    uint32_t src[V];
#pragma unroll
    for (int v = 0; v < V; ++v) src[v] = ntt_automorph_src(p0 + (uint32_t)v, g, log_n);
    const W* bq = a.key_b[t] + ko;
    const W* aq = a.key_a[t] + ko;
    for (uint32_t s = 0; s < Ls; ++s) {
      const W* ds = dp + (uint64_t)s * limb_words;
      W xv[V], bv[V], av[V];
#pragma unroll
      for (int v = 0; v < V; ++v) xv[v] = ds[src[v]];
      ld_vec<W, VEC, V>(bv, bq + (uint64_t)s * N);
      ld_vec<W, VEC, V>(av, aq + (uint64_t)s * N);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        s0[v] = add_mod<W>(s0[v], mont_mul<W>(xv[v], bv[v], lc.q, lc.qinv), lc.q);
        s1[v] = add_mod<W>(s1[v], mont_mul<W>(xv[v], av[v], lc.q, lc.qinv), lc.q);
      }
    }
  }
  st_vec<W, VEC, V>(acc0 + o, s0);
  st_vec<W, VEC, V>(acc1 + o, s1);
}

// The coefficient-domain addend of a rotate-and-sum over the ciphertext's
// limbs: out[i] = z x[i] + sum_{t < nt} +-x[i g_t^-1 mod 2N] (k_automorph_odd's
// gather summed over the steps of a launch), canonical; z x is x added z times.
// x at limb stride x_ls, out at the chunk's own (limb_words).  ACC: added to
// what out holds.  Grid as k_elementwise, one word per thread.
struct RotsumC0Args {
  uint32_t ginv[ROTSUM_T];
};
template <class W, bool ACC>
__global__ void __launch_bounds__(256)
k_rotsum_c0(W* out, const W* __restrict__ x, RotsumC0Args a, TabPtrs<W> tp, uint32_t log_n, uint64_t limb_words,
            uint64_t x_ls, uint32_t nt, uint32_t z) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= limb_words) return;
  const uint32_t l = blockIdx.y;
  const W q = tp.lc[l].q;
  const uint64_t N = 1ull << log_n;
  const uint32_t jo = (uint32_t)(i & (N - 1));
  const W* xp = x + (uint64_t)l * x_ls + (i - jo);
  W s = ACC ? out[(uint64_t)l * limb_words + i] : (W)0;
  if (z != 0) {  // (uniform)
    const W c = xp[jo];
    for (uint32_t r = 0; r < z; ++r) s = add_mod<W>(s, c, q);
  }
  for (uint32_t t = 0; t < nt; ++t) {  // (uniform)
    const uint32_t e = (jo * a.ginv[t]) & (uint32_t)(2 * N - 1);
    W c = xp[e & (uint32_t)(N - 1)];
    if (e >= N) c = c == 0 ? (W)0 : (W)(q - c);
    s = add_mod<W>(s, c, q);
  }
  out[(uint64_t)l * limb_words + i] = s;
}

// A lane's vector of sigma_g(x) in the NTT domain, x one plane: the V source
// positions src[] of V consecutive positions lie in ONE aligned vector (the map
// is block-structured), permuted inside.  VEC: that vector is loaded whole and
// the words picked in registers (selects on the low bits, no indexed register
// file); else V = 1 and it is the word itself.
template <class W, bool VEC, int V>
__device__ __forceinline__ void ld_gather_vec(W (&o)[V], const W* plane, const uint32_t (&src)[V]) {
  if constexpr (VEC) {
    W w[V];
    ld_vec<W, VEC, V>(w, plane + (src[0] & ~(uint32_t)(V - 1)));
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const uint32_t e = src[v] & (uint32_t)(V - 1);
      W r = w[0];
#pragma unroll
      for (int u = 1; u < V; ++u) r = e == (uint32_t)u ? w[u] : r;
      o[v] = r;
    }
  } else {
    o[0] = plane[src[0]];
  }
}

// The inner sums of the double-hoisted transform (rnt_ct_linear_bsgs_hybrid_dh)
// in the NTT domain over E, both components of nj <= DH_JT giants and nb <=
// DH_BT babies in one launch:
//   out0[jj] (+)= sum_b m[jj][b] (.) sigma_{g_b}(T0_b + P c0^),  out1[jj] with T1_b
// T0_b / T1_b ([L][B][N], canonical) are the hoisted key products of baby b
// BEFORE any ModDown, read through the NTT-domain permutation of sigma_{g_b}
// (ntt_automorph_src: aligned vectors onto aligned vectors), so the rotated
// blocks are never written.  P c0^ enters on the limbs j < Lv alone, from the
// transformed ciphertext (c0h, c1h: [Lv][B][N]) through the same permutation:
// mont_mul(c, P 2^w) = [P]_{q_j} c.  A baby with t0[b] == nullptr is a step of
// 0: (P c0^, P c1^) at the lane's own position, nothing on the special limbs.
// m points at plane (jj = 0, b = 0) of the plaintexts over E in their PLAIN
// NTT-domain form (limb stride m_ls, giant stride m_row, baby stride N, one
// plane for every poly of the batch); the Montgomery products x m 2^-w are
// summed canonically and every sum is multiplied ONCE by 2^w mod q in the
// epilogue (k_plain_mac's rule), so the plaintexts take no pass of their own.
// `accum` (uniform): added to what the outputs hold (the baby groups after the
// first).  Grid as k_hoist_mac; a lane owns one vector position of one limb
// and 2 DH_JT sums.
constexpr int DH_JT = (int)kDhJt;
constexpr int DH_BT = (int)kDhBt;

template <class W>
struct DhMacArgs {
  const W* t0[DH_BT];
  const W* t1[DH_BT];
  uint32_t g[DH_BT];
  W* out0[DH_JT];
  W* out1[DH_JT];
};
template <class W, bool VEC>
__global__ void __launch_bounds__(256)
k_dh_bsgs_mac(DhMacArgs<W> a, const W* __restrict__ c0h, const W* __restrict__ c1h, const W* __restrict__ m,
              const W* __restrict__ Pw, TabPtrs<W> tp, uint32_t log_n, uint64_t limb_words, uint64_t m_ls,
              uint64_t m_row, uint32_t nb, uint32_t nj, uint32_t Lv, uint32_t accum, LimbMap lm) {
  constexpr int V = VEC ? 16 / (int)sizeof(W) : 1;
  const uint32_t j = blockIdx.y;
  const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (i >= limb_words) return;
  const LimbConst<W> lc = tp.lc[root_limb(j, lm)];
  const uint64_t N = 1ull << log_n;
  const uint32_t p0 = (uint32_t)(i & (N - 1));  // V divides N: one plane
  const uint64_t o = (uint64_t)j * limb_words + i;
  const uint64_t plane = o - p0;
  const bool ql = j < Lv;  // (uniform)
  const W pw = ql ? Pw[j] : (W)0;
  const W* mp = m + (uint64_t)j * m_ls + p0;
  W s0[DH_JT][V], s1[DH_JT][V];
#pragma unroll
  for (int jj = 0; jj < DH_JT; ++jj)
#pragma unroll
    for (int v = 0; v < V; ++v) s0[jj][v] = s1[jj][v] = (W)0;
  for (uint32_t b = 0; b < nb; ++b) {  // (uniform)
    W x0[V], x1[V];
    if (a.t0[b] == nullptr) {  // (uniform) a step of 0
      if (!ql) continue;
      W u0[V], u1[V];
      ld_vec<W, VEC, V>(u0, c0h + o);
      ld_vec<W, VEC, V>(u1, c1h + o);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        x0[v] = mont_mul<W>(u0[v], pw, lc.q, lc.qinv);
        x1[v] = mont_mul<W>(u1[v], pw, lc.q, lc.qinv);
      }
    } else {
      const uint32_t g = a.g[b];
      uint32_t src[V];
#pragma unroll
      for (int v = 0; v < V; ++v) src[v] = ntt_automorph_src(p0 + (uint32_t)v, g, log_n);
      ld_gather_vec<W, VEC, V>(x0, a.t0[b] + plane, src);
      ld_gather_vec<W, VEC, V>(x1, a.t1[b] + plane, src);
      if (ql) {
        W u0[V];
        ld_gather_vec<W, VEC, V>(u0, c0h + plane, src);
#pragma unroll
        for (int v = 0; v < V; ++v) x0[v] = add_mod<W>(x0[v], mont_mul<W>(u0[v], pw, lc.q, lc.qinv), lc.q);
      }
    }
    const W* mb = mp + (uint64_t)b * N;
#pragma unroll
    for (int jj = 0; jj < DH_JT; ++jj) {
      if ((uint32_t)jj < nj) {  // (uniform)
        W mv[V];
        ld_vec<W, VEC, V>(mv, mb + (uint64_t)jj * m_row);
#pragma unroll
        for (int v = 0; v < V; ++v) {
          s0[jj][v] = add_mod<W>(s0[jj][v], mont_mul<W>(x0[v], mv[v], lc.q, lc.qinv), lc.q);
          s1[jj][v] = add_mod<W>(s1[jj][v], mont_mul<W>(x1[v], mv[v], lc.q, lc.qinv), lc.q);
        }
      }
    }
  }
#pragma unroll
  for (int jj = 0; jj < DH_JT; ++jj) {
    if ((uint32_t)jj < nj) {  // (uniform)
#pragma unroll
      for (int v = 0; v < V; ++v) {
        s0[jj][v] = shoup_mul<W>(s0[jj][v], lc.rmod, lc.rmod_p, lc.q);
        s1[jj][v] = shoup_mul<W>(s1[jj][v], lc.rmod, lc.rmod_p, lc.q);
      }
      if (accum) {  // (uniform)
        W q0[V], q1[V];
        ld_vec<W, VEC, V>(q0, a.out0[jj] + o);
        ld_vec<W, VEC, V>(q1, a.out1[jj] + o);
#pragma unroll
        for (int v = 0; v < V; ++v) {
          s0[jj][v] = add_mod<W>(q0[v], s0[jj][v], lc.q);
          s1[jj][v] = add_mod<W>(q1[v], s1[jj][v], lc.q);
        }
      }
      st_vec<W, VEC, V>(a.out0[jj] + o, s0[jj]);
      st_vec<W, VEC, V>(a.out1[jj] + o, s1[jj]);
    }
  }
}

// The fold of the inner sums into the giant accumulators of the double-hoisted
// transform, over E in the NTT domain:
//   A0 (+)= sum_{jj: g = 0} v0[jj] + sum_{jj: g != 0} sigma_g(v0[jj]),  A1 (+)= sum_{jj: g = 0} v1[jj]
// for nj <= DH_JT giants (g[jj] == 0: a giant step of 0), sigma_g the gather
// above.  The second components of the rotating giants are not read: they go
// through ModDown and the giant key instead, whose products k_hoist_mac_acc
// then adds to A0 / A1.  ACC: added to what A0 / A1 hold (the giant groups
// after the first); else the launch initialises both.  Every operand is a
// block of the call's own workspace, 16-byte aligned with whole vectors in a
// plane, so the kernel has the 16-byte form alone (the launcher refuses
// anything else).
template <class W>
struct DhFoldArgs {
  const W* v0[DH_JT];
  const W* v1[DH_JT];
  uint32_t g[DH_JT];
};
template <class W, bool ACC>
__global__ void __launch_bounds__(256)
k_dh_bsgs_fold(W* A0, W* A1, DhFoldArgs<W> a, TabPtrs<W> tp, uint32_t log_n, uint64_t limb_words, uint32_t nj,
               LimbMap lm) {
  constexpr bool VEC = true;
  constexpr int V = 16 / (int)sizeof(W);
  const uint32_t j = blockIdx.y;
  const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (i >= limb_words) return;
  const W q = tp.lc[root_limb(j, lm)].q;
  const uint64_t N = 1ull << log_n;
  const uint32_t p0 = (uint32_t)(i & (N - 1));  // V divides N: one plane
  const uint64_t o = (uint64_t)j * limb_words + i;
  const uint64_t plane = o - p0;
  W s0[V], s1[V];
  if constexpr (ACC) {
    ld_vec<W, VEC, V>(s0, A0 + o);
    ld_vec<W, VEC, V>(s1, A1 + o);
  } else {
#pragma unroll
    for (int v = 0; v < V; ++v) s0[v] = s1[v] = (W)0;
  }
  for (uint32_t jj = 0; jj < nj; ++jj) {  // (uniform)
    const uint32_t g = a.g[jj];
    W x[V];
    if (g == 0) {  // (uniform)
      W y[V];
      ld_vec<W, VEC, V>(x, a.v0[jj] + o);
      ld_vec<W, VEC, V>(y, a.v1[jj] + o);
#pragma unroll
      for (int v = 0; v < V; ++v) s1[v] = add_mod<W>(s1[v], y[v], q);
    } else {
      uint32_t src[V];
#pragma unroll
      for (int v = 0; v < V; ++v) src[v] = ntt_automorph_src(p0 + (uint32_t)v, g, log_n);
      ld_gather_vec<W, VEC, V>(x, a.v0[jj] + plane, src);
    }
#pragma unroll
    for (int v = 0; v < V; ++v) s0[v] = add_mod<W>(s0[v], x[v], q);
  }
  st_vec<W, VEC, V>(A0 + o, s0);
  st_vec<W, VEC, V>(A1 + o, s1);
}


// ModUp of the hybrid key-switch: digit d = blockIdx.y owns the cnt <= alpha
// source limbs from d alpha on.  A thread reads its vector of each of them
// once, takes y_i = x_i (Q_d/q_i)^-1 mod q_i, and writes for every limb t of
// the key basis (tp: its tables, LE limbs) sum_i y_i conv[d][i][t] mod m_t with
// conv = (Q_d/q_i) 2^w mod m_t: the fast base conversion in Montgomery form.
// For t in the digit the constant row is one-hot -- Q_d/q_i = 0 mod q_t for
// i != t, and y_t (Q_d/q_t) = x_t -- so the same sum stores x_t 2^w exactly
// and no lane branches on t.  y_i < q_i may exceed m_t: the Shoup product takes
// any word.  D is [LE][gridDim.y][B][N].  AMAX >= alpha keeps the y_i in
// registers (the unrolled loop's `a < cnt` is uniform); AMAX == 0 serves any
// alpha by recomputing y_i per target limb (the re-reads hit the cache).
// blockIdx.z takes a run of tper target limbs: one run at large batches, several
// where one ciphertext's vectors alone would leave most of the CUs idle.
template <class W, bool VEC, int AMAX>
__global__ void __launch_bounds__(256)
k_modup(W* __restrict__ D, const W* __restrict__ x, TabPtrs<W> tp, const W* __restrict__ yinv,
        const W* __restrict__ yinvp, const W* __restrict__ conv, const W* __restrict__ convp,
        uint64_t limb_words, uint64_t src_ls, uint32_t alpha, uint32_t Lv, uint32_t LE, uint32_t tper,
        LimbMap lm) {
  constexpr int V = VEC ? 16 / (int)sizeof(W) : 1;
  const uint32_t d = blockIdx.y;
  const uint32_t t0 = blockIdx.z * tper;
  const uint32_t t1 = t0 + tper < LE ? t0 + tper : LE;
  const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (i >= limb_words) return;
  const uint32_t first = d * alpha;
  const uint32_t cnt = Lv - first < alpha ? Lv - first : alpha;
  const W* xp = x + (uint64_t)first * src_ls + i;
  const W* crow = conv + (uint64_t)d * alpha * LE;
  const W* prow = convp + (uint64_t)d * alpha * LE;
  W y[AMAX > 0 ? AMAX : 1][V];
  if constexpr (AMAX > 0) {
#pragma unroll
    for (int a = 0; a < AMAX; ++a) {
      if ((uint32_t)a < cnt) {  // (uniform)
        W xv[V];
        ld_vec<W, VEC, V>(xv, xp + (uint64_t)a * src_ls);
        const W q = tp.lc[root_limb(first + a, lm)].q, c = yinv[first + a], cp = yinvp[first + a];
#pragma unroll
        for (int v = 0; v < V; ++v) y[a][v] = shoup_mul<W>(xv[v], c, cp, q);
      }
    }
  }
  for (uint32_t t = t0; t < t1; ++t) {
    const W q = tp.lc[root_limb(t, lm)].q;
    W acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = (W)0;
    if constexpr (AMAX > 0) {
#pragma unroll
      for (int a = 0; a < AMAX; ++a) {
        if ((uint32_t)a < cnt) {
          const W c = crow[(uint64_t)a * LE + t], cp = prow[(uint64_t)a * LE + t];
#pragma unroll
          for (int v = 0; v < V; ++v) acc[v] = add_mod<W>(acc[v], shoup_mul<W>(y[a][v], c, cp, q), q);
        }
      }
    } else {
      for (uint32_t a = 0; a < cnt; ++a) {
        W xv[V];
        ld_vec<W, VEC, V>(xv, xp + (uint64_t)a * src_ls);
        const W qs = tp.lc[root_limb(first + a, lm)].q, ci = yinv[first + a], cip = yinvp[first + a];
        const W c = crow[(uint64_t)a * LE + t], cp = prow[(uint64_t)a * LE + t];
#pragma unroll
        for (int v = 0; v < V; ++v)
          acc[v] = add_mod<W>(acc[v], shoup_mul<W>(shoup_mul<W>(xv[v], ci, cip, qs), c, cp, q), q);
      }
    }
    st_vec<W, VEC, V>(D + ((uint64_t)t * gridDim.y + d) * limb_words + i, acc);
  }
}

// ModDown of the hybrid key-switch: A is a coefficient-domain accumulator over
// the key basis ([Lv + K][B][N] at limb stride a_ls, tp its tables).  A thread
// reads its vector of the K special planes once, z_k = A_{p_k} (P/p_k)^-1 mod
// p_k, and writes for every ciphertext limb j < Lv
//   out_j = (A_j - sum_k z_k (P/p_k mod q_j)) P^-1 mod q_j  (+ add_j),
// canonical, at limb stride out_ls (the addend, optional and uniform, at
// add_ls).  z_k < p_k may exceed q_j: Shoup products.  KMAX as k_modup's AMAX;
// blockIdx.y takes a run of jper output limbs, as k_modup's blockIdx.z.
template <class W, bool VEC, int KMAX>
__global__ void __launch_bounds__(256)
k_moddown(W* __restrict__ out, uint64_t out_ls, const W* __restrict__ A, uint64_t a_ls, const W* add,
          uint64_t add_ls, TabPtrs<W> tp, const W* __restrict__ pinv, const W* __restrict__ pinvp,
          const W* __restrict__ pq, const W* __restrict__ pqp, const W* __restrict__ Pinv,
          const W* __restrict__ Pinvp, uint64_t limb_words, uint32_t Lv, uint32_t K, uint32_t jper, LimbMap lm) {
  constexpr int V = VEC ? 16 / (int)sizeof(W) : 1;
  const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (i >= limb_words) return;
  const uint32_t j0 = blockIdx.y * jper;
  const uint32_t j1 = j0 + jper < Lv ? j0 + jper : Lv;
  const W* sp = A + (uint64_t)Lv * a_ls + i;
  W z[KMAX > 0 ? KMAX : 1][V];
  if constexpr (KMAX > 0) {
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if ((uint32_t)k < K) {  // (uniform)
        W av[V];
        ld_vec<W, VEC, V>(av, sp + (uint64_t)k * a_ls);
        const W p = tp.lc[root_limb(Lv + k, lm)].q, c = pinv[k], cp = pinvp[k];
#pragma unroll
        for (int v = 0; v < V; ++v) z[k][v] = shoup_mul<W>(av[v], c, cp, p);
      }
    }
  }
  for (uint32_t j = j0; j < j1; ++j) {
    const W q = tp.lc[root_limb(j, lm)].q;
    W cv[V];
#pragma unroll
    for (int v = 0; v < V; ++v) cv[v] = (W)0;
    if constexpr (KMAX > 0) {
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        if ((uint32_t)k < K) {
          const W c = pq[(uint64_t)k * Lv + j], cp = pqp[(uint64_t)k * Lv + j];
#pragma unroll
          for (int v = 0; v < V; ++v) cv[v] = add_mod<W>(cv[v], shoup_mul<W>(z[k][v], c, cp, q), q);
        }
      }
    } else {
      for (uint32_t k = 0; k < K; ++k) {
        W av[V];
        ld_vec<W, VEC, V>(av, sp + (uint64_t)k * a_ls);
        const W p = tp.lc[root_limb(Lv + k, lm)].q, ci = pinv[k], cip = pinvp[k];
        const W c = pq[(uint64_t)k * Lv + j], cp = pqp[(uint64_t)k * Lv + j];
#pragma unroll
        for (int v = 0; v < V; ++v)
          cv[v] = add_mod<W>(cv[v], shoup_mul<W>(shoup_mul<W>(av[v], ci, cip, p), c, cp, q), q);
      }
    }
    W av[V], r[V];
    ld_vec<W, VEC, V>(av, A + (uint64_t)j * a_ls + i);
    const W c = Pinv[j], cp = Pinvp[j];
#pragma unroll
    for (int v = 0; v < V; ++v) r[v] = shoup_mul<W>(av[v] - cv[v] + q, c, cp, q);  // a - conv + q in (0, 2q)
    if (add != nullptr) {  // (uniform)
      W dv[V];
      ld_vec<W, VEC, V>(dv, add + (uint64_t)j * add_ls + i);
#pragma unroll
      for (int v = 0; v < V; ++v) r[v] = add_mod<W>(r[v], dv[v], q);
    }
    st_vec<W, VEC, V>(out + (uint64_t)j * out_ls + i, r);
  }
}

// One limb of k_moddown for a lane: r = (A_j - sum_k z_k (P/p_k mod q_j)) P^-1
// (+ add_j) mod q_j, canonical -- the statements of k_moddown's loop body, for
// k_moddown_rescale, which needs them at two places.
template <class W, bool VEC, int KMAX, int V>
__device__ __forceinline__ void moddown_limb(W (&r)[V], uint32_t j, const W (&z)[KMAX > 0 ? KMAX : 1][V],
                                             const W* __restrict__ A, uint64_t a_ls, const W* add, uint64_t add_ls,
                                             const TabPtrs<W>& tp, const W* __restrict__ pinv,
                                             const W* __restrict__ pinvp, const W* __restrict__ pq,
                                             const W* __restrict__ pqp, const W* __restrict__ Pinv,
                                             const W* __restrict__ Pinvp, uint64_t i, uint32_t Lv, uint32_t K, LimbMap lm) {
  const W q = tp.lc[root_limb(j, lm)].q;
  W cv[V];
#pragma unroll
  for (int v = 0; v < V; ++v) cv[v] = (W)0;
  if constexpr (KMAX > 0) {
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if ((uint32_t)k < K) {  // (uniform)
        const W c = pq[(uint64_t)k * Lv + j], cp = pqp[(uint64_t)k * Lv + j];
#pragma unroll
        for (int v = 0; v < V; ++v) cv[v] = add_mod<W>(cv[v], shoup_mul<W>(z[k][v], c, cp, q), q);
      }
    }
  } else {
    const W* sp = A + (uint64_t)Lv * a_ls + i;
    for (uint32_t k = 0; k < K; ++k) {
      W av[V];
      ld_vec<W, VEC, V>(av, sp + (uint64_t)k * a_ls);
      const W p = tp.lc[root_limb(Lv + k, lm)].q, ci = pinv[k], cip = pinvp[k];
      const W c = pq[(uint64_t)k * Lv + j], cp = pqp[(uint64_t)k * Lv + j];
#pragma unroll
      for (int v = 0; v < V; ++v)
        cv[v] = add_mod<W>(cv[v], shoup_mul<W>(shoup_mul<W>(av[v], ci, cip, p), c, cp, q), q);
    }
  }
  W av[V];
  ld_vec<W, VEC, V>(av, A + (uint64_t)j * a_ls + i);
  const W c = Pinv[j], cp = Pinvp[j];
#pragma unroll
  for (int v = 0; v < V; ++v) r[v] = shoup_mul<W>(av[v] - cv[v] + q, c, cp, q);  // a - conv + q in (0, 2q)
  if (add != nullptr) {  // (uniform)
    W dv[V];
    ld_vec<W, VEC, V>(dv, add + (uint64_t)j * add_ls + i);
#pragma unroll
    for (int v = 0; v < V; ++v) r[v] = add_mod<W>(r[v], dv[v], q);
  }
}

// k_moddown followed by k_rescale, the level-Lv result never written: a lane
// takes its z_k once, r_last = limb Lv - 1 of ModDown(A) (+ add), canonical,
// and stores for every limb j < Lv - 1 of its run
//   out_j = (r_j - [r_last]_{q_j}) (q_last mod q_j)^-1 mod q_j
// with r_j as k_moddown computes it, [r_last]_{q_j} reduced as k_rescale reduces
// it (Shoup product by 1) and rinv / rinvp the row of the ciphertext basis'
// rescale table k_rescale reads: the words of the two kernels in sequence.
// blockIdx.y takes a run of jper of the Lv - 1 output limbs; every run
// recomputes z_k and r_last (K + 1 planes read again, hits of the cache).
//
// AFFINE (rnt_ct_mul_relin_rescale_affine_hybrid): the output word o_j of a
// lane is held back and
//   out_j = w o_j + u z_j (+ b on coefficient 0 of a poly)  mod q_j,
// canonical, is stored in its place -- z the addend at limb stride z_ls (null:
// no second term), w, u, b signed integers by value.  Their residues mod q_j
// are formed per limb from LimbConst alone (affine_residue: Shoup products by
// 1, no division; uniform, so once a wave) and w, u go to Montgomery form
// (times 2^w mod q_j, LimbConst::rmod), so a word costs two Montgomery
// products and an addition and no table is read: nothing is copied from the
// host.  The bias belongs to element 0 of the lane whose position is a
// multiple of N (k_lincomb's rule; V divides N where VEC); the caller passes
// b = 0 for component 1.  A lane loads z_j at its position before it stores
// out_j there and no other lane touches that position, so z may be out (the
// AFFINE instantiations have no __restrict__ on out).
template <class W>
struct MdAffineArg {
  const W* z;
  uint64_t z_ls;
  int64_t w, u, b;
  uint32_t nmask;  // N - 1
};

// |c| < 2^63 mod q, canonical and without a division: Shoup products by 1.
template <class W>
__device__ __forceinline__ W affine_residue(int64_t c, const LimbConst<W>& lc) {
  const uint64_t m = c < 0 ? (uint64_t)(-(c + 1)) + 1u : (uint64_t)c;
  W r;
  if constexpr (sizeof(W) == 4) r = mag_mod<W>(m, lc);
  else r = shoup_mul<W>((W)m, (W)1, lc.one_p, lc.q);
  return c < 0 && r != 0 ? (W)(lc.q - r) : r;
}

template <class W, bool AFFINE>
struct MdOut { using type = W* __restrict__; };
template <class W>
struct MdOut<W, true> { using type = W*; };

template <class W, bool VEC, int KMAX, bool AFFINE = false>
__global__ void __launch_bounds__(256)
k_moddown_rescale(typename MdOut<W, AFFINE>::type out, uint64_t out_ls, const W* __restrict__ A, uint64_t a_ls,
                  const W* add, uint64_t add_ls, TabPtrs<W> tp, const W* __restrict__ pinv, const W* __restrict__ pinvp,
                  const W* __restrict__ pq, const W* __restrict__ pqp, const W* __restrict__ Pinv,
                  const W* __restrict__ Pinvp, const W* __restrict__ rinv, const W* __restrict__ rinvp,
                  uint64_t limb_words, uint32_t Lv, uint32_t K, uint32_t jper, LimbMap lm, MdAffineArg<W> af) {
  constexpr int V = VEC ? 16 / (int)sizeof(W) : 1;
  const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (i >= limb_words) return;
  const uint32_t last = Lv - 1;
  const uint32_t j0 = blockIdx.y * jper;
  const uint32_t j1 = j0 + jper < last ? j0 + jper : last;
  W z[KMAX > 0 ? KMAX : 1][V];
  if constexpr (KMAX > 0) {
    const W* sp = A + (uint64_t)Lv * a_ls + i;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if ((uint32_t)k < K) {  // (uniform)
        W av[V];
        ld_vec<W, VEC, V>(av, sp + (uint64_t)k * a_ls);
        const W p = tp.lc[root_limb(Lv + k, lm)].q, c = pinv[k], cp = pinvp[k];
#pragma unroll
        for (int v = 0; v < V; ++v) z[k][v] = shoup_mul<W>(av[v], c, cp, p);
      }
    }
  }
  W rl[V];
  moddown_limb<W, VEC, KMAX, V>(rl, last, z, A, a_ls, add, add_ls, tp, pinv, pinvp, pq, pqp, Pinv, Pinvp, i, Lv, K, lm);
  for (uint32_t j = j0; j < j1; ++j) {
    W r[V], o[V];
    moddown_limb<W, VEC, KMAX, V>(r, j, z, A, a_ls, add, add_ls, tp, pinv, pinvp, pq, pqp, Pinv, Pinvp, i, Lv, K, lm);
    const LimbConst<W> lc = tp.lc[root_limb(j, lm)];
    const W inv = rinv[j], invp = rinvp[j];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const W cl = shoup_mul<W>(rl[v], (W)1, lc.one_p, lc.q);  // canonical r_last mod q_j, as k_rescale's
      o[v] = shoup_mul<W>(sub_mod<W>(r[v], cl, lc.q), inv, invp, lc.q);
    }
    if constexpr (AFFINE) {
      const W wm = shoup_mul<W>(affine_residue<W>(af.w, lc), lc.rmod, lc.rmod_p, lc.q);  // w 2^w mod q_j (uniform)
#pragma unroll
      for (int v = 0; v < V; ++v) o[v] = mont_mul<W>(o[v], wm, lc.q, lc.qinv);
      if (af.z != nullptr) {  // (uniform)
        const W um = shoup_mul<W>(affine_residue<W>(af.u, lc), lc.rmod, lc.rmod_p, lc.q);
        W zv[V];
        ld_vec<W, VEC, V>(zv, af.z + (uint64_t)j * af.z_ls + i);
#pragma unroll
        for (int v = 0; v < V; ++v) o[v] = add_mod<W>(o[v], mont_mul<W>(zv[v], um, lc.q, lc.qinv), lc.q);
      }
      if (((uint32_t)i & af.nmask) == 0) o[0] = add_mod<W>(o[0], affine_residue<W>(af.b, lc), lc.q);
    }
    st_vec<W, VEC, V>(out + (uint64_t)j * out_ls + i, o);
  }
}

// k_hoist_mac for one step whose sums start from a seed: on a ciphertext limb
// j < Lv, acc0 from seed_b[j] c_j and acc1 from seed_a[j] c_j with c_j = P 2^w
// mod q_j (Pw / Pwp, Shoup); on a special limb from 0 (the branch on
// blockIdx.y is uniform).  The seeds are the tensor's d0^ 2^-w, d1^ 2^-w (NTT
// domain, limb stride seed_ls), so seed c_j = NTT(P d) on limb j and the sums
// are the accumulators of A + P d, whose ModDown is ModDown(A) + d: the seeds
// need no inverse transform and ModDown no addend.  One accumulator pair, not
// HOIST_T: the multiply has one key.  A kernel of its own, so that k_hoist_mac
// stays as it is.  A lane reads its seed vectors before it stores the sums at
// the same (limb, position), so with seed_ls = limb_words the seeds may lie in
// the accumulators' own first Lv limbs (seed_b == out0, seed_a == out1: no
// __restrict__ on the four).
template <class W, bool VEC>
__global__ void __launch_bounds__(256)
k_hoist_mac_seed(W* out0, W* out1, const W* __restrict__ key_b,
                 const W* __restrict__ key_a, const W* __restrict__ d, const W* seed_b,
                 const W* seed_a, uint64_t seed_ls, const W* __restrict__ Pw,
                 const W* __restrict__ Pwp, TabPtrs<W> tp, uint32_t log_n, uint64_t limb_words, uint64_t key_ls,
                 uint32_t Ls, uint32_t Lv, LimbMap lm) {
  constexpr int V = VEC ? 16 / (int)sizeof(W) : 1;
  const uint32_t j = blockIdx.y;
  const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (i >= limb_words) return;
  const uint32_t rj = root_limb(j, lm);
  const LimbConst<W> lc = tp.lc[rj];
  const uint64_t N = 1ull << log_n;
  const W* dp = d + (uint64_t)j * Ls * limb_words + i;
  const uint64_t ko = (uint64_t)rj * key_ls + (i & (N - 1));  // V divides N: one plane
  W acc0[V], acc1[V];
  if (j < Lv) {  // (uniform)
    W s0[V], s1[V];
    ld_vec<W, VEC, V>(s0, seed_b + (uint64_t)j * seed_ls + i);
    ld_vec<W, VEC, V>(s1, seed_a + (uint64_t)j * seed_ls + i);
    const W c = Pw[j], cp = Pwp[j];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      acc0[v] = shoup_mul<W>(s0[v], c, cp, lc.q);
      acc1[v] = shoup_mul<W>(s1[v], c, cp, lc.q);
    }
  } else {
#pragma unroll
    for (int v = 0; v < V; ++v) acc0[v] = acc1[v] = (W)0;
  }
  for (uint32_t s = 0; s < Ls; ++s) {
    W xv[V], bv[V], av[V];
    ld_vec<W, VEC, V>(xv, dp + (uint64_t)s * limb_words);
    ld_vec<W, VEC, V>(bv, key_b + ko + (uint64_t)s * N);
    ld_vec<W, VEC, V>(av, key_a + ko + (uint64_t)s * N);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      acc0[v] = add_mod<W>(acc0[v], mont_mul<W>(xv[v], bv[v], lc.q, lc.qinv), lc.q);
      acc1[v] = add_mod<W>(acc1[v], mont_mul<W>(xv[v], av[v], lc.q, lc.qinv), lc.q);
    }
  }
  const uint64_t g = (uint64_t)j * limb_words + i;
  st_vec<W, VEC, V>(out0 + g, acc0);
  st_vec<W, VEC, V>(out1 + g, acc1);
}


// k_moddown followed by sigma_g of the result (g odd), written at the output's
// own limb stride: the per-step tail of the hoisted hybrid rotation, out =
// sigma_g(ModDown(A) (+ add)).  Position i of a plane lands at t mod N with
// t = i g mod 2N, negated mod q_j when t >= N (zero stays zero).  A SCATTER:
// the K special planes, A_j and the addend stay 16-byte vector streams and only
// the Lv result planes are written a word at a time.  A gather would read the
// K + Lv (+ Lv addend) input planes a word at a time -- (K + 2 Lv) / Lv times
// the element-granular instructions, the K special ones again for every run of
// a split grid -- and put their latency in front of the arithmetic, where a
// store retires behind it.  g is odd, so i -> i g mod 2N is a bijection of the
// positions: every output word is written exactly once, no ordering needed.
// xcd_gid()'s deal gives every XCD whole polys, so the partial lines of a
// result plane (N words, at most 1 MiB) meet in ONE L2 before they leave it.
// The output must not overlap A or the addend.
template <class W, bool VEC, int KMAX>
__global__ void __launch_bounds__(256)
k_moddown_auto(W* __restrict__ out, uint64_t out_ls, const W* __restrict__ A, uint64_t a_ls,
               const W* __restrict__ add, uint64_t add_ls, TabPtrs<W> tp, const W* __restrict__ pinv,
               const W* __restrict__ pinvp, const W* __restrict__ pq, const W* __restrict__ pqp,
               const W* __restrict__ Pinv, const W* __restrict__ Pinvp, uint64_t limb_words, uint32_t log_n,
               uint32_t g, uint32_t Lv, uint32_t K, uint32_t jper, LimbMap lm) {
  constexpr int V = VEC ? 16 / (int)sizeof(W) : 1;
  const uint64_t i = xcd_gid() * V;
  if (i >= limb_words) return;
  const uint32_t j0 = blockIdx.y * jper;
  const uint32_t j1 = j0 + jper < Lv ? j0 + jper : Lv;
  const uint32_t N = 1u << log_n;
  const uint32_t pos = (uint32_t)i & (N - 1);  // V divides N: one plane
  uint64_t dst[V];
  bool neg[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const uint32_t t = ((pos + (uint32_t)v) * g) & (2 * N - 1);  // (mod 2^32 first: 2N divides it)
    neg[v] = t >= N;
    dst[v] = (i - pos) + (t & (N - 1));
  }
  const W* sp = A + (uint64_t)Lv * a_ls + i;
  W z[KMAX > 0 ? KMAX : 1][V];
  if constexpr (KMAX > 0) {
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if ((uint32_t)k < K) {  // (uniform)
        W av[V];
        ld_vec<W, VEC, V>(av, sp + (uint64_t)k * a_ls);
        const W p = tp.lc[root_limb(Lv + k, lm)].q, c = pinv[k], cp = pinvp[k];
#pragma unroll
        for (int v = 0; v < V; ++v) z[k][v] = shoup_mul<W>(av[v], c, cp, p);
      }
    }
  }
  for (uint32_t j = j0; j < j1; ++j) {
    const W q = tp.lc[root_limb(j, lm)].q;
    W cv[V];
#pragma unroll
    for (int v = 0; v < V; ++v) cv[v] = (W)0;
    if constexpr (KMAX > 0) {
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        if ((uint32_t)k < K) {
          const W c = pq[(uint64_t)k * Lv + j], cp = pqp[(uint64_t)k * Lv + j];
#pragma unroll
          for (int v = 0; v < V; ++v) cv[v] = add_mod<W>(cv[v], shoup_mul<W>(z[k][v], c, cp, q), q);
        }
      }
    } else {
      for (uint32_t k = 0; k < K; ++k) {
        W av[V];
        ld_vec<W, VEC, V>(av, sp + (uint64_t)k * a_ls);
        const W p = tp.lc[root_limb(Lv + k, lm)].q, ci = pinv[k], cip = pinvp[k];
        const W c = pq[(uint64_t)k * Lv + j], cp = pqp[(uint64_t)k * Lv + j];
#pragma unroll
        for (int v = 0; v < V; ++v)
          cv[v] = add_mod<W>(cv[v], shoup_mul<W>(shoup_mul<W>(av[v], ci, cip, p), c, cp, q), q);
      }
    }
    W av[V], r[V];
    ld_vec<W, VEC, V>(av, A + (uint64_t)j * a_ls + i);
    const W c = Pinv[j], cp = Pinvp[j];
#pragma unroll
    for (int v = 0; v < V; ++v) r[v] = shoup_mul<W>(av[v] - cv[v] + q, c, cp, q);  // a - conv + q in (0, 2q)
    if (add != nullptr) {  // (uniform)
      W dv[V];
      ld_vec<W, VEC, V>(dv, add + (uint64_t)j * add_ls + i);
#pragma unroll
      for (int v = 0; v < V; ++v) r[v] = add_mod<W>(r[v], dv[v], q);
    }
    W* op = out + (uint64_t)j * out_ls;
#pragma unroll
    for (int v = 0; v < V; ++v) op[dst[v]] = neg[v] && r[v] != 0 ? (W)(q - r[v]) : r[v];
  }
}

// rescale_into (poly.rs:212-225): out[l] = (c_l - (c_last mod q_l)) * q_last^-1.
template <class W>
__global__ void __launch_bounds__(256)
k_rescale(W* __restrict__ out, const W* __restrict__ in, const W* __restrict__ lastp,
          const W* __restrict__ inv_t, const W* __restrict__ invp_t, TabPtrs<W> tp,
          uint64_t ls_in, uint64_t ls_out, uint64_t poly_words, uint32_t limbs) {
  // one thread per coefficient position over every kept limb: c_last is read
  // once per position, not once per limb (the per-(limb, position) form read
  // the last plane L - 1 times)
  const uint64_t off = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (off >= poly_words) return;
  const W last = lastp[off];
#pragma unroll 4
  for (uint32_t l = 0; l < limbs; ++l) {
    const LimbConst<W> lc = tp.lc[l];
    const W inv = inv_t[l];  // (q_last mod q_l)^-1 mod q_l
    const W invp = invp_t[l];
    const W ci = in[(uint64_t)l * ls_in + off];
    const W cl = shoup_mul<W>(last, (W)1, lc.one_p, lc.q);  // canonical c_last mod q_l (R5)
    out[(uint64_t)l * ls_out + off] = shoup_mul<W>(sub_mod<W>(ci, cl, lc.q), inv, invp, lc.q);
  }
}

// Scalar linear combinations of ciphertexts (rnt_ct_lincomb[_rescale]): with
// x_i the n_in terms of a ciphertext component ([Lv][n_in B][N], term i of
// ciphertext b at poly i B + b, so at + i ct_words of a limb plane),
//   r_j = sum_i w[t][j][i] x_i (+ bias[t][j] X^0 on component 0)  mod q_t,
// canonical, for the n_out outputs j ([.][n_out B][N], output j at + j
// ct_words).  A lane owns one vector of the B N positions of a ciphertext
// batch; blockIdx.z is the component (a uniform choice of pointers).  For each
// limb t of its run it loads its n_in vectors once, forms the n_out sums one
// after the other (Shoup products by the wave-uniform weights w / wp, read
// through scalar registers) and stores them: every input plane is read once a
// run, every output plane written once.  RESCALE: the lane first forms
// r_last[j] on limb Lv - 1 for every j and then stores
//   out_j = (r_j - [r_last_j]_{q_t}) (q_last mod q_t)^-1 mod q_t,  t < Lv - 1,
// reduced as k_rescale reduces it (Shoup product by 1; rinv / rinvp the row of
// the rescale table k_rescale reads): the words of the un-rescaled kernel
// followed by k_rescale, the sums never written.  blockIdx.y takes a run of
// tper limbs; with RESCALE every run recomputes r_last (n_in planes read again,
// hits of the cache).  The NI >= n_in input vectors of a limb live in registers
// (the unrolled loop's guard is uniform); the loop over the outputs is a
// runtime one, so the code does not grow with n_out and the weights of one
// output are the only scalars held.  The n_out last-limb sums of a lane wait in
// LDS, 16 bytes per lane and output (lc_rl[j][lane]: lanes side by side, no
// bank conflict; each lane reads back only what it wrote, so no barrier).  The
// bias belongs to coefficient 0 of every poly: element 0 of the lane whose
// position is a multiple of N (V divides N where VEC).
struct LincombGeom {
  uint64_t ct_words, in_ls, out_ls;
  uint32_t n_in, n_out, Lv, tper, nmask;
};

template <class W, bool VEC, int NI, int V>
__device__ __forceinline__ void lincomb_load(W (&xv)[NI][V], const W* __restrict__ xp, uint64_t ct_words,
                                             uint32_t n_in) {
#pragma unroll
  for (int ii = 0; ii < NI; ++ii)
    if ((uint32_t)ii < n_in) ld_vec<W, VEC, V>(xv[ii], xp + (uint64_t)ii * ct_words);  // (uniform)
}

// Output j's sum on limb t for a lane: wrow = the weights of (t, j).
template <class W, int NI, int V>
__device__ __forceinline__ void lincomb_sum(W (&r)[V], const W (&xv)[NI][V], const W* __restrict__ wrow,
                                            const W* __restrict__ wprow, uint32_t n_in, W bias, W q) {
#pragma unroll
  for (int v = 0; v < V; ++v) r[v] = (W)0;
#pragma unroll
  for (int ii = 0; ii < NI; ++ii) {
    if ((uint32_t)ii < n_in) {  // (uniform)
      const W c = wrow[ii], cp = wprow[ii];
#pragma unroll
      for (int v = 0; v < V; ++v) r[v] = add_mod<W>(r[v], shoup_mul<W>(xv[ii][v], c, cp, q), q);
    }
  }
  r[0] = add_mod<W>(r[0], bias, q);
}

extern __shared__ uint4 lc_rl[];  // RESCALE: [n_out][256] last-limb sums, one 16-byte slot per lane

template <class W, bool VEC, bool RESCALE, int NI>
__global__ void __launch_bounds__(256)
k_lincomb(W* __restrict__ out0, W* __restrict__ out1, const W* __restrict__ x0, const W* __restrict__ x1,
          const W* __restrict__ w, const W* __restrict__ wp, const W* __restrict__ bias,
          const W* __restrict__ rinv, const W* __restrict__ rinvp, LincombGeom a, TabPtrs<W> tp) {
  // w, wp: [Lv][n_out][n_in] weights and Shoup companions; bias: [Lv][n_out] or nullptr; rinv, rinvp
  // (RESCALE): (q_last mod q_t)^-1 mod q_t and companions.  All __restrict__ parameters: the outputs
  // alias none of them, so the uniform reads stay scalar loads after the first store.
  constexpr int V = VEC ? 16 / (int)sizeof(W) : 1;
  const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (i >= a.ct_words) return;
  const uint32_t comp = blockIdx.z;
  const W* x = (comp ? x1 : x0) + i;
  W* out = (comp ? out1 : out0) + i;
  const bool biased = comp == 0 && bias != nullptr;           // (uniform)
  const bool bias_lane = biased && ((uint32_t)i & a.nmask) == 0;  // coefficient 0 of a poly
  const uint32_t lo = RESCALE ? a.Lv - 1 : a.Lv;
  const uint32_t t0 = blockIdx.y * a.tper;
  const uint32_t t1 = t0 + a.tper < lo ? t0 + a.tper : lo;
  const uint32_t wstride = a.n_out * a.n_in;
  W xv[NI][V];
  if constexpr (RESCALE) {
    const uint32_t last = a.Lv - 1;
    const W q = tp.lc[last].q;
    lincomb_load<W, VEC, NI, V>(xv, x + (uint64_t)last * a.in_ls, a.ct_words, a.n_in);
#pragma unroll 1
    for (uint32_t j = 0; j < a.n_out; ++j) {
      const uint32_t wj = last * a.n_out + j;
      const W b = biased ? bias[wj] : (W)0;
      W r[V];
      lincomb_sum<W, NI, V>(r, xv, w + (uint64_t)wj * a.n_in, wp + (uint64_t)wj * a.n_in, a.n_in,
                            bias_lane ? b : (W)0, q);
      uint4 slot = make_uint4(0, 0, 0, 0);
      __builtin_memcpy(&slot, r, sizeof(r));
      lc_rl[j * 256 + threadIdx.x] = slot;
    }
  }
  for (uint32_t t = t0; t < t1; ++t) {
    const LimbConst<W> lc = tp.lc[t];
    lincomb_load<W, VEC, NI, V>(xv, x + (uint64_t)t * a.in_ls, a.ct_words, a.n_in);
    const W* wrow = w + (uint64_t)t * wstride;
    const W* wprow = wp + (uint64_t)t * wstride;
    W* op = out + (uint64_t)t * a.out_ls;
    W inv = (W)0, invp = (W)0;
    if constexpr (RESCALE) {
      inv = rinv[t];
      invp = rinvp[t];
    }
#pragma unroll 1
    for (uint32_t j = 0; j < a.n_out; ++j) {
      const W b = biased ? bias[t * a.n_out + j] : (W)0;
      W r[V];
      lincomb_sum<W, NI, V>(r, xv, wrow + j * a.n_in, wprow + j * a.n_in, a.n_in, bias_lane ? b : (W)0, lc.q);
      if constexpr (RESCALE) {
        const uint4 slot = lc_rl[j * 256 + threadIdx.x];
        W rl[V];
        __builtin_memcpy(rl, &slot, sizeof(rl));
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const W cl = shoup_mul<W>(rl[v], (W)1, lc.one_p, lc.q);  // canonical r_last mod q_t, as k_rescale's
          r[v] = shoup_mul<W>(sub_mod<W>(r[v], cl, lc.q), inv, invp, lc.q);
        }
      }
      st_vec<W, VEC, V>(op + (uint64_t)j * a.ct_words, r);
    }
  }
}

// The accumulated tensor of rnt_ct_dot_relin[_rescale]_hybrid: with x0^, x1^,
// y0^, y1^ the forward-transformed planes of a group of nt <= DOT_T terms
// ([L][nt c][N] at limb stride in_ls, term i of the chunk's c ciphertexts at
// + i term_words of a limb plane),
//   d0^ = sum_i x0^_i y0^_i   d1^ = sum_i (x0^_i y1^_i + x1^_i y0^_i)
//   d2^ = sum_i x1^_i y1^_i,
// each scaled by 2^-w (Montgomery products of plain NTT words: the seed
// convention k_hoist_mac_seed consumes and k_tensor_rows produces), at limb
// stride out_ls.  A lane owns one vector of the c N positions of the chunk on
// limb blockIdx.y and loops over the terms; with `accum` (uniform) the sums
// are added to the words already stored, so a group after the first extends
// the sums of the groups before it.  SQ: y is x (a sum of squares), two loads
// a term and d1^ = sum_i 2 x0^_i x1^_i.  Every product is reduced
// (mont_mul: a, b < q -> < q) and every sum is an add_mod of two canonical
// words, so no bound depends on the modulus or on the number of terms.  The
// loop over the DOT_T terms is unrolled behind a uniform guard, so the loads of
// the next terms are issued under the products of this one.
constexpr int DOT_T = (int)kDotT;
struct DotGeom {
  uint64_t limb_words, term_words, in_ls, out_ls;
  uint32_t nt, accum;
};
template <class W, bool VEC, bool SQ>
__global__ void __launch_bounds__(256)
k_dot_tensor(W* __restrict__ d0, W* __restrict__ d1, W* __restrict__ d2, const W* __restrict__ x0,
             const W* __restrict__ x1, const W* y0, const W* y1, DotGeom a, TabPtrs<W> tp, LimbMap lm) {
  // (y0, y1 without __restrict__: with SQ they are x0, x1 and are not read)
  constexpr int V = VEC ? 16 / (int)sizeof(W) : 1;
  const uint32_t l = blockIdx.y;
  const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (i >= a.limb_words) return;
  const LimbConst<W> lc = tp.lc[root_limb(l, lm)];
  const uint64_t in = (uint64_t)l * a.in_ls + i;
  W s0[V], s1[V], s2[V];
#pragma unroll
  for (int v = 0; v < V; ++v) s0[v] = s1[v] = s2[v] = (W)0;
#pragma unroll
  for (int tt = 0; tt < DOT_T; ++tt) {
    if ((uint32_t)tt < a.nt) {  // (uniform)
      const uint64_t g = in + (uint64_t)tt * a.term_words;
      W a0[V], a1[V];
      ld_vec<W, VEC, V>(a0, x0 + g);
      ld_vec<W, VEC, V>(a1, x1 + g);
      if constexpr (SQ) {
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const W c = mont_mul<W>(a0[v], a1[v], lc.q, lc.qinv);
          s0[v] = add_mod<W>(s0[v], mont_mul<W>(a0[v], a0[v], lc.q, lc.qinv), lc.q);
          s1[v] = add_mod<W>(s1[v], add_mod<W>(c, c, lc.q), lc.q);
          s2[v] = add_mod<W>(s2[v], mont_mul<W>(a1[v], a1[v], lc.q, lc.qinv), lc.q);
        }
      } else {
        W b0[V], b1[V];
        ld_vec<W, VEC, V>(b0, y0 + g);
        ld_vec<W, VEC, V>(b1, y1 + g);
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const W c = add_mod<W>(mont_mul<W>(a0[v], b1[v], lc.q, lc.qinv),
                                 mont_mul<W>(a1[v], b0[v], lc.q, lc.qinv), lc.q);
          s0[v] = add_mod<W>(s0[v], mont_mul<W>(a0[v], b0[v], lc.q, lc.qinv), lc.q);
          s1[v] = add_mod<W>(s1[v], c, lc.q);
          s2[v] = add_mod<W>(s2[v], mont_mul<W>(a1[v], b1[v], lc.q, lc.qinv), lc.q);
        }
      }
    }
  }
  const uint64_t o = (uint64_t)l * a.out_ls + i;
  if (a.accum) {  // (uniform)
    W p0[V], p1[V], p2[V];
    ld_vec<W, VEC, V>(p0, d0 + o);
    ld_vec<W, VEC, V>(p1, d1 + o);
    ld_vec<W, VEC, V>(p2, d2 + o);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      s0[v] = add_mod<W>(p0[v], s0[v], lc.q);
      s1[v] = add_mod<W>(p1[v], s1[v], lc.q);
      s2[v] = add_mod<W>(p2[v], s2[v], lc.q);
    }
  }
  st_vec<W, VEC, V>(d0 + o, s0);
  st_vec<W, VEC, V>(d1 + o, s1);
  st_vec<W, VEC, V>(d2 + o, s2);
}

// The plaintext sums of rnt_ct_plain_mac[_rescale]: with x0^, x1^ the
// forward-transformed planes of a group of nt <= PLAIN_T terms (term i of the
// chunk's c ciphertexts at + i term_words of a limb plane, limb stride in_ls)
// and m^ the NTT-domain plaintexts where the caller keeps them (term i at
// + i m_term_words of a limb plane, limb stride m_ls),
//   s0^ = sum_i x0^_i m^_i (+ bias^)   s1^ = sum_i x1^_i m^_i
// as canonical NTT-domain words at limb stride out_ls.  A lane owns one vector
// of the c N positions of the chunk on limb blockIdx.y; its plaintext words
// are at position & m_mask of the term's plane (N - 1: one plaintext for every
// ciphertext; all ones: one per ciphertext), the bias' at position & b_mask.
// The products are Montgomery products of plain words (x m 2^-w, reduced) and
// the sums add_mod of canonical words, so no bound depends on the modulus or on
// the number of terms; each sum is then multiplied once by 2^w mod q
// (LimbConst::rmod), so neither the plaintexts nor the sums take a pass of
// their own.  With `accum` (uniform) the canonical sums of the groups before
// are added after that factor; the bias (nullptr: none) goes to s0^ of the
// last group.  The loop over the PLAIN_T terms is unrolled behind a uniform
// guard: no counter or address arithmetic between the terms, and the three
// loads of a term are in flight together.  (The compiler keeps each guarded
// term a block of its own, so the registers do not grow with PLAIN_T:
// DESIGN.md §4 has the table.)
constexpr int PLAIN_T = (int)kPlainT;
struct PlainMacGeom {
  uint64_t limb_words, term_words, in_ls, out_ls, m_term_words, m_ls, m_mask, b_ls, b_mask;
  uint32_t nt, accum;
};
template <class W, bool VEC>
__global__ void __launch_bounds__(256)
k_plain_mac(W* __restrict__ d0, W* __restrict__ d1, const W* __restrict__ x0, const W* __restrict__ x1,
            const W* __restrict__ m, const W* __restrict__ bias, PlainMacGeom a, TabPtrs<W> tp, LimbMap lm) {
  constexpr int V = VEC ? 16 / (int)sizeof(W) : 1;
  const uint32_t l = blockIdx.y;
  const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (i >= a.limb_words) return;
  const LimbConst<W> lc = tp.lc[root_limb(l, lm)];
  const uint64_t in = (uint64_t)l * a.in_ls + i;
  const uint64_t mi = (uint64_t)l * a.m_ls + (i & a.m_mask);
  W s0[V], s1[V];
#pragma unroll
  for (int v = 0; v < V; ++v) s0[v] = s1[v] = (W)0;
#pragma unroll
  for (int tt = 0; tt < PLAIN_T; ++tt) {
    if ((uint32_t)tt < a.nt) {  // (uniform)
      const uint64_t g = in + (uint64_t)tt * a.term_words;
      W a0[V], a1[V], p[V];
      ld_vec<W, VEC, V>(a0, x0 + g);
      ld_vec<W, VEC, V>(a1, x1 + g);
      ld_vec<W, VEC, V>(p, m + mi + (uint64_t)tt * a.m_term_words);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        s0[v] = add_mod<W>(s0[v], mont_mul<W>(a0[v], p[v], lc.q, lc.qinv), lc.q);
        s1[v] = add_mod<W>(s1[v], mont_mul<W>(a1[v], p[v], lc.q, lc.qinv), lc.q);
      }
    }
  }
#pragma unroll
  for (int v = 0; v < V; ++v) {
    s0[v] = shoup_mul<W>(s0[v], lc.rmod, lc.rmod_p, lc.q);
    s1[v] = shoup_mul<W>(s1[v], lc.rmod, lc.rmod_p, lc.q);
  }
  const uint64_t o = (uint64_t)l * a.out_ls + i;
  if (a.accum) {  // (uniform)
    W p0[V], p1[V];
    ld_vec<W, VEC, V>(p0, d0 + o);
    ld_vec<W, VEC, V>(p1, d1 + o);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      s0[v] = add_mod<W>(p0[v], s0[v], lc.q);
      s1[v] = add_mod<W>(p1[v], s1[v], lc.q);
    }
  }
  if (bias != nullptr) {  // (uniform)
    W b[V];
    ld_vec<W, VEC, V>(b, bias + (uint64_t)l * a.b_ls + (i & a.b_mask));
#pragma unroll
    for (int v = 0; v < V; ++v) s0[v] = add_mod<W>(s0[v], b[v], lc.q);
  }
  st_vec<W, VEC, V>(d0 + o, s0);
  st_vec<W, VEC, V>(d1 + o, s1);
}


// automorphism for odd g: out[t] gathers its unique source (poly.rs:520-537).
template <class W>
__global__ void __launch_bounds__(256)
k_automorph_odd(W* __restrict__ out, const W* __restrict__ in, TabPtrs<W> tp, uint32_t log_n,
                uint64_t ginv, uint64_t poly_words, uint64_t total) {
  const uint64_t i = xcd_gid();
  if (i >= poly_words) return;
  const uint64_t N = 1ull << log_n;
  const uint32_t l = blockIdx.y;
  const uint64_t gid = (uint64_t)l * poly_words + i;
  const uint64_t jo = i & (N - 1);
  const uint64_t pbase = gid - jo;
  const uint64_t t = (jo * ginv) & (2 * N - 1);
  const W q = tp.lc[l].q;
  W v;
  if (t < N) {
    v = in[pbase + t];
  } else {
    const W c = in[pbase + t - N];
    v = c == 0 ? (W)0 : (W)(q - c);
  }
  out[gid] = v;
}

// automorphism for even g != 0 mod 2N (not a ring automorphism): the
// reference's scatter loop keeps, per output slot, the LAST (largest i)
// non-zero writer (poly.rs:520-537).  g = 2^e * h, h odd; i*g = r (mod 2N)
// iff 2^e | r and i = (r >> e) * h^-1 (mod M), M = 2N >> e.
template <class W>
__global__ void __launch_bounds__(256)
k_automorph_even(W* __restrict__ out, const W* __restrict__ in, TabPtrs<W> tp, uint32_t log_n,
                 uint32_t e, uint64_t hinv, uint64_t poly_words, uint64_t total) {
  const uint64_t i = xcd_gid();
  if (i >= poly_words) return;
  const uint64_t N = 1ull << log_n;
  const uint32_t l = blockIdx.y;
  const uint64_t gid = (uint64_t)l * poly_words + i;
  const uint64_t jo = i & (N - 1);
  const uint64_t pbase = gid - jo;
  const uint64_t M = (2 * N) >> e;
  const W q = tp.lc[l].q;
  int64_t best = -1;
  int best_neg = 0;
  W best_val = 0;
  for (int h = 0; h < 2; ++h) {
    const uint64_t r = jo + (h ? N : 0);
    if (r & ((1ull << e) - 1)) continue;
    const uint64_t i0 = ((r >> e) * hinv) & (M - 1);
    if (i0 >= N) continue;
    // largest i = i0 + k*M < N with a non-zero coefficient
    uint64_t kmax = (N - 1 - i0) / M;
    for (int64_t k = (int64_t)kmax; k >= 0; --k) {
      const uint64_t i = i0 + (uint64_t)k * M;
      if ((int64_t)i <= best) break;
      const W c = in[pbase + i];
      if (c != 0) {
        best = (int64_t)i;
        best_neg = h;
        best_val = c;
        break;
      }
    }
  }
  W v = 0;
  if (best >= 0) v = best_neg ? (W)(q - best_val) : best_val;
  out[gid] = v;
}

__device__ __forceinline__ uint64_t brv_dev(uint64_t k, uint32_t bits) {
  return bits == 0 ? 0 : (__brevll(k) >> (64 - bits));
}

// host [B][L][N] u64 staging -> device [L][B][N] W (with validation).
template <class W>
__global__ void __launch_bounds__(256)
k_import(W* __restrict__ dst, const uint64_t* __restrict__ stage, TabPtrs<W> tp, uint32_t log_n,
         uint32_t L, uint64_t ls, int to_brv, unsigned long long* err, uint64_t total) {
  const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= total) return;
  const uint64_t N = 1ull << log_n;
  const uint64_t k = gid & (N - 1);
  const uint64_t pl = gid >> log_n;  // p*L + l
  const uint32_t l = (uint32_t)(pl % L);
  const uint64_t p = pl / L;
  const uint64_t v = stage[gid];
  const uint64_t q = (uint64_t)tp.lc[l].q;
  if (v >= q) atomicMin(err, (unsigned long long)gid);
  const uint64_t pos = to_brv ? brv_dev(k, log_n) : k;
  dst[(uint64_t)l * ls + p * N + pos] = (W)(v >= q ? 0 : v);
}

// from_coeffs (poly.rs:55-61): rem_euclid per channel.
template <class W>
__global__ void __launch_bounds__(256)
k_import_coeffs(W* __restrict__ dst, const int64_t* __restrict__ coeffs, TabPtrs<W> tp,
                uint32_t L, uint64_t ls, uint64_t total) {
  // one thread per coefficient ([B][N] = the [L][B][N] offset within a
  // limb): read it once, write its residue into every limb
  const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= total) return;
  const int64_t c = coeffs[gid];
  for (uint32_t l = 0; l < L; ++l) dst[(uint64_t)l * ls + gid] = rem_euclid<W>(c, tp.lc[l]);
}

template <class W>
__global__ void __launch_bounds__(256)
k_export(uint64_t* __restrict__ stage, const W* __restrict__ src, uint32_t log_n, uint32_t L,
         uint64_t ls, int from_brv, uint64_t total) {
  const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= total) return;
  const uint64_t N = 1ull << log_n;
  const uint64_t k = gid & (N - 1);
  const uint64_t pl = gid >> log_n;
  const uint32_t l = (uint32_t)(pl % L);
  const uint64_t p = pl / L;
  const uint64_t pos = from_brv ? brv_dev(k, log_n) : k;
  stage[gid] = (uint64_t)src[(uint64_t)l * ls + p * N + pos];
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

// The streaming launchers share one shape (rnt_launch.hpp): argument checks
// (hipErrorInvalidValue), the empty launch (hipSuccess), `vec` from vec_ok(),
// grid x from blocks_x() under grid_ok() (hipErrorInvalidConfiguration), then
// by_word / with_bool / with_tier pick the kernel's instantiation.
hipError_t launch_elementwise(const Launch& k, int op, void* out, const void* a, const void* b) {
  return by_word(k, [&](auto w) -> hipError_t {
    using W = decltype(w);
    const uint64_t limb_words = (uint64_t)k.B << k.t->log_n;
    if (limb_words == 0 || k.L == 0) return hipSuccess;
    // (a limb's words, not a plane's: the kernel's vectors need not stay within a poly)
    const bool vec = vec_ok<W>(limb_words, {}, ptr_bits(out, a, b));
    const uint64_t bx = blocks_x<W>(limb_words, vec);
    if (!grid_ok(bx, k.L)) return hipErrorInvalidConfiguration;
    const dim3 grid((unsigned)bx, (unsigned)k.L);
    with_tier<0, 1, 2, 3, 4>((unsigned)op, [&](auto OP) {  // (any other op: 4)
      with_bool(vec, [&](auto VEC) {
        hipLaunchKernelGGL((k_elementwise<W, decltype(OP)::value, decltype(VEC)::value>), grid, dim3(256), 0, k.s, (W*)out, (const W*)a,
                           (const W*)b, tab_ptrs<W>(k.t), limb_words);
      });
    });
    return hipGetLastError();
  });
}

hipError_t launch_bcast_mul(const Launch& k, int kind, void* out, const void* x, const void* m, uint64_t m_ls,
                            bool accum) {
  return by_word(k, [&](auto w) -> hipError_t {
    using W = decltype(w);
    const uint64_t N = 1ull << k.t->log_n;
    const uint64_t limb_words = (uint64_t)k.B * N;
    if (limb_words == 0 || k.L == 0) return hipSuccess;
    // 16-byte accesses: whole vectors within a plane, every plane 16-byte aligned
    const bool vec = vec_ok<W>(N, {m_ls}, ptr_bits(out, x, m));
    const uint64_t bx = blocks_x<W>(limb_words, vec);
    if (!grid_ok(bx, k.L)) return hipErrorInvalidConfiguration;
    const dim3 grid((unsigned)bx, (unsigned)k.L);
    with_tier<0, 1>((unsigned)kind, [&](auto KIND) {
      with_bool(vec, [&](auto VEC) {
        hipLaunchKernelGGL((k_bcast_mul<W, decltype(KIND)::value, decltype(VEC)::value>), grid, dim3(256), 0, k.s, (W*)out,
                           (const W*)x, (const W*)m, tab_ptrs<W>(k.t), k.t->log_n, limb_words, m_ls, accum ? 1u : 0u);
      });
    });
    return hipGetLastError();
  });
}

hipError_t launch_bsgs_mac(const Launch& k, void* const* outs, uint32_t nj, uint32_t accum_mask, const void* x,
                           uint64_t blk_words, const void* m, uint64_t m_ls, uint32_t n_baby) {
  return by_word(k, [&](auto w) -> hipError_t {
    using W = decltype(w);
    const uint64_t N = 1ull << k.t->log_n;
    const uint64_t limb_words = (uint64_t)k.B * N;
    if (nj == 0 || nj > (uint32_t)BSGS_JT || n_baby == 0 || blk_words < (uint64_t)k.L * limb_words)
      return hipErrorInvalidValue;
    if (limb_words == 0 || k.L == 0) return hipSuccess;
    BsgsOuts<W> o{};
    uintptr_t align = ptr_bits(x, m);
    for (uint32_t jj = 0; jj < nj; ++jj) {
      o.out[jj] = (W*)outs[jj];
      align |= ptr_bits(outs[jj]);
    }
    // 16-byte accesses: whole vectors within a plane, every plane and block 16-byte aligned
    const bool vec = vec_ok<W>(N, {m_ls, blk_words}, align);
    const uint64_t bx = blocks_x<W>(limb_words, vec);
    if (!grid_ok(bx, k.L)) return hipErrorInvalidConfiguration;
    const dim3 grid((unsigned)bx, (unsigned)k.L, 2);
    with_bool(vec, [&](auto VEC) {
      hipLaunchKernelGGL((k_bsgs_mac<W, decltype(VEC)::value>), grid, dim3(256), 0, k.s, o, (const W*)x, (const W*)m,
                         tab_ptrs<W>(k.t), k.t->log_n, limb_words, blk_words, m_ls, n_baby, nj, accum_mask);
    });
    return hipGetLastError();
  });
}

template <class W>
static hipError_t mont_one_t(const Launch& k, void* out) {
  const uint64_t N = 1ull << k.t->log_n;
  if (k.L == 0) return hipSuccess;
  if (k.L > 65535) return hipErrorInvalidConfiguration;
  hipLaunchKernelGGL((k_mont_one<W>), dim3((unsigned)((N + 255) / 256), (unsigned)k.L), dim3(256), 0, k.s,
                     (W*)out, tab_ptrs<W>(k.t), k.t->log_n);
  return hipGetLastError();
}

hipError_t launch_hoist_digits(const Launch& k, void* D, const void* c1, uint64_t src_ls) {
  return by_word(k, [&](auto w) -> hipError_t {
    using W = decltype(w);
    const uint64_t N = 1ull << k.t->log_n;
    const uint64_t limb_words = (uint64_t)k.B * N;
    const size_t Ls = k.src_limbs();
    if (limb_words == 0 || k.L == 0 || Ls == 0) return hipSuccess;
    if (src_ls < limb_words) return hipErrorInvalidValue;
    // 16-byte accesses: whole vectors within a plane, every plane 16-byte aligned
    const bool vec = vec_ok<W>(N, {src_ls}, ptr_bits(D, c1));
    const uint64_t bx = blocks_x<W>(limb_words, vec);
    if (!grid_ok(bx, Ls)) return hipErrorInvalidConfiguration;
    const dim3 grid((unsigned)bx, (unsigned)Ls);
    with_bool(vec, [&](auto VEC) {
      hipLaunchKernelGGL((k_hoist_digits<W, decltype(VEC)::value>), grid, dim3(256), 0, k.s, (W*)D, (const W*)c1,
                         tab_ptrs<W>(k.t), limb_words, src_ls, (uint32_t)k.L);
    });
    return hipGetLastError();
  });
}

// accum: k_hoist_mac_acc, the sums added to what acc0[t] / acc1[t] hold.
static hipError_t hoist_mac(const Launch& k, void* const* acc0, void* const* acc1, uint32_t nt, const void* d,
                            const void* const* key_a, const void* const* key_b, uint64_t key_ls, bool accum) {
  return by_word(k, [&](auto w) -> hipError_t {
    using W = decltype(w);
    const uint64_t N = 1ull << k.t->log_n;
    const uint64_t limb_words = (uint64_t)k.B * N;
    const size_t Ls = k.src_limbs();
    if (nt == 0 || nt > (uint32_t)HOIST_T || Ls == 0 || key_ls < Ls * N || !limb_map_ok(k))
      return hipErrorInvalidValue;
    if (limb_words == 0 || k.L == 0) return hipSuccess;
    HoistArgs<W> a{};
    uintptr_t align = ptr_bits(d);
    for (uint32_t t = 0; t < nt; ++t) {
      a.key_a[t] = (const W*)key_a[t];
      a.key_b[t] = (const W*)key_b[t];
      a.acc0[t] = (W*)acc0[t];
      a.acc1[t] = (W*)acc1[t];
      align |= ptr_bits(key_a[t], key_b[t], acc0[t], acc1[t]);
    }
    // 16-byte accesses: whole vectors within a plane, every plane and block 16-byte aligned
    const bool vec = vec_ok<W>(N, {key_ls}, align);
    const uint64_t bx = blocks_x<W>(limb_words, vec);
    if (!grid_ok(bx, k.L)) return hipErrorInvalidConfiguration;
    const dim3 grid((unsigned)bx, (unsigned)k.L);
    with_bool(accum, [&](auto ACC) {
      with_bool(vec, [&](auto VEC) {
        constexpr auto kernel = decltype(ACC)::value ? k_hoist_mac_acc<W, decltype(VEC)::value>
                                                     : k_hoist_mac<W, decltype(VEC)::value>;
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, k.s, a, (const W*)d, tab_ptrs<W>(k.t), k.t->log_n, limb_words,
                           key_ls, (uint32_t)Ls, nt, limb_map(k));
      });
    });
    return hipGetLastError();
  });
}
hipError_t launch_hoist_mac(const Launch& k, void* const* acc0, void* const* acc1, uint32_t nt, const void* d,
                            const void* const* key_a, const void* const* key_b, uint64_t key_ls) {
  return hoist_mac(k, acc0, acc1, nt, d, key_a, key_b, key_ls, false);
}
hipError_t launch_hoist_mac_acc(const Launch& k, void* const* acc0, void* const* acc1, uint32_t nt, const void* d,
                                const void* const* key_a, const void* const* key_b, uint64_t key_ls) {
  return hoist_mac(k, acc0, acc1, nt, d, key_a, key_b, key_ls, true);
}

static uint64_t inv_mod_pow2(uint64_t h, uint64_t M);

hipError_t launch_automorphism_ntt(const Launch& k, void* out, const void* in, uint64_t g) {
  return by_word(k, [&](auto w) -> hipError_t {
    using W = decltype(w);
    const uint64_t N = 1ull << k.t->log_n;
    const uint64_t limb_words = (uint64_t)k.B * N;
    if ((g & 1) == 0 || out == in) return hipErrorInvalidValue;
    if (limb_words == 0 || k.L == 0) return hipSuccess;
    const uint64_t bx = blocks_x<W>(limb_words, false);
    if (!grid_ok(bx, k.L)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL((k_automorph_ntt<W>), dim3((unsigned)bx, (unsigned)k.L), dim3(256), 0, k.s, (W*)out,
                       (const W*)in, k.t->log_n, (uint32_t)(g & (2 * N - 1)), limb_words);
    return hipGetLastError();
  });
}

hipError_t launch_rotsum_mac(const Launch& k, void* acc0, void* acc1, uint32_t nt, const uint64_t* g, const void* d,
                             const void* const* key_a, const void* const* key_b, uint64_t key_ls, bool accum) {
  return by_word(k, [&](auto w) -> hipError_t {
    using W = decltype(w);
    const uint64_t N = 1ull << k.t->log_n;
    const uint64_t limb_words = (uint64_t)k.B * N;
    const size_t Ls = k.src_limbs();
    if (nt == 0 || nt > (uint32_t)ROTSUM_T || Ls == 0 || key_ls < Ls * N || !limb_map_ok(k))
      return hipErrorInvalidValue;
    if (limb_words == 0 || k.L == 0) return hipSuccess;
    RotsumArgs<W> a{};
    uintptr_t align = ptr_bits(d, acc0, acc1);
    for (uint32_t t = 0; t < nt; ++t) {
      if ((g[t] & 1) == 0) return hipErrorInvalidValue;
      a.key_a[t] = (const W*)key_a[t];
      a.key_b[t] = (const W*)key_b[t];
      a.g[t] = (uint32_t)(g[t] & (2 * N - 1));
      align |= ptr_bits(key_a[t], key_b[t]);
    }
    // 16-byte accesses: whole vectors within a plane, every plane and block 16-byte aligned
    const bool vec = vec_ok<W>(N, {key_ls}, align);
    const uint64_t bx = blocks_x<W>(limb_words, vec);
    if (!grid_ok(bx, k.L)) return hipErrorInvalidConfiguration;
    const dim3 grid((unsigned)bx, (unsigned)k.L);
    with_bool(accum, [&](auto ACC) {
      with_bool(vec, [&](auto VEC) {
        hipLaunchKernelGGL((k_rotsum_mac<W, decltype(VEC)::value, decltype(ACC)::value>), grid, dim3(256), 0, k.s,
                           (W*)acc0, (W*)acc1, a, (const W*)d, tab_ptrs<W>(k.t), k.t->log_n, limb_words, key_ls,
                           (uint32_t)Ls, nt, limb_map(k));
      });
    });
    return hipGetLastError();
  });
}

hipError_t launch_rotsum_c0(const Launch& k, void* out, const void* x, uint64_t x_ls, uint32_t nt, const uint64_t* g,
                            uint32_t z, bool accum) {
  return by_word(k, [&](auto w) -> hipError_t {
    using W = decltype(w);
    const uint64_t N = 1ull << k.t->log_n;
    const uint64_t limb_words = (uint64_t)k.B * N;
    if (nt > (uint32_t)ROTSUM_T || x_ls < limb_words || out == x) return hipErrorInvalidValue;
    if (limb_words == 0 || k.L == 0) return hipSuccess;
    RotsumC0Args a{};
    for (uint32_t t = 0; t < nt; ++t) {
      if ((g[t] & 1) == 0) return hipErrorInvalidValue;
      a.ginv[t] = (uint32_t)inv_mod_pow2(g[t] & (2 * N - 1), 2 * N);
    }
    const uint64_t bx = blocks_x<W>(limb_words, false);
    if (!grid_ok(bx, k.L)) return hipErrorInvalidConfiguration;
    with_bool(accum, [&](auto ACC) {
      hipLaunchKernelGGL((k_rotsum_c0<W, decltype(ACC)::value>), dim3((unsigned)bx, (unsigned)k.L), dim3(256), 0, k.s,
                         (W*)out, (const W*)x, a, tab_ptrs<W>(k.t), k.t->log_n, limb_words, x_ls, nt, z);
    });
    return hipGetLastError();
  });
}

hipError_t launch_dh_bsgs_mac(const Launch& k, void* const* out0, void* const* out1, uint32_t nj, const void* const* t0,
                              const void* const* t1, const uint64_t* g, uint32_t nb, const void* c0h, const void* c1h,
                              const void* m, uint64_t m_ls, uint64_t m_row, bool accum, const HybridConsts& hc) {
  return by_word(k, [&](auto w) -> hipError_t {
    using W = decltype(w);
    const uint64_t N = 1ull << k.t->log_n;
    const uint64_t limb_words = (uint64_t)k.B * N;
    if (nj == 0 || nj > (uint32_t)DH_JT || nb == 0 || nb > (uint32_t)DH_BT || hc.Lv == 0 ||
        k.L != (size_t)hc.Lv + hc.K || !limb_map_ok(k) || !c0h || !c1h || !m || !hc.Pw || m_row < (uint64_t)nb * N ||
        m_ls < (nj - 1) * m_row + (uint64_t)nb * N)
      return hipErrorInvalidValue;
    if (limb_words == 0) return hipSuccess;
    DhMacArgs<W> a{};
    uintptr_t align = ptr_bits(c0h, c1h, m);
    for (uint32_t b = 0; b < nb; ++b) {
      if ((t0[b] == nullptr) != (t1[b] == nullptr)) return hipErrorInvalidValue;
      if (t0[b] && (g[b] & 1) == 0) return hipErrorInvalidValue;
      a.t0[b] = (const W*)t0[b];
      a.t1[b] = (const W*)t1[b];
      a.g[b] = (uint32_t)(g[b] & (2 * N - 1));
      align |= ptr_bits(t0[b], t1[b]);
    }
    for (uint32_t jj = 0; jj < nj; ++jj) {
      if (!out0[jj] || !out1[jj]) return hipErrorInvalidValue;
      a.out0[jj] = (W*)out0[jj];
      a.out1[jj] = (W*)out1[jj];
      align |= ptr_bits(out0[jj], out1[jj]);
    }
    // 16-byte accesses: whole vectors within a plane, every plane and block 16-byte aligned
    const bool vec = vec_ok<W>(N, {m_ls, m_row}, align);
    const uint64_t bx = blocks_x<W>(limb_words, vec);
    if (!grid_ok(bx, k.L)) return hipErrorInvalidConfiguration;
    const dim3 grid((unsigned)bx, (unsigned)k.L);
    with_bool(vec, [&](auto VEC) {
      hipLaunchKernelGGL((k_dh_bsgs_mac<W, decltype(VEC)::value>), grid, dim3(256), 0, k.s, a, (const W*)c0h,
                         (const W*)c1h, (const W*)m, (const W*)hc.Pw, tab_ptrs<W>(k.t), k.t->log_n, limb_words, m_ls,
                         m_row, nb, nj, hc.Lv, accum ? 1u : 0u, limb_map(k));
    });
    return hipGetLastError();
  });
}

hipError_t launch_dh_bsgs_fold(const Launch& k, void* A0, void* A1, const void* const* v0, const void* const* v1,
                               const uint64_t* g, uint32_t nj, bool accum) {
  return by_word(k, [&](auto w) -> hipError_t {
    using W = decltype(w);
    const uint64_t N = 1ull << k.t->log_n;
    const uint64_t limb_words = (uint64_t)k.B * N;
    if (nj == 0 || nj > (uint32_t)DH_JT || !limb_map_ok(k) || !A0 || !A1) return hipErrorInvalidValue;
    if (limb_words == 0 || k.L == 0) return hipSuccess;
    DhFoldArgs<W> a{};
    uintptr_t align = ptr_bits(A0, A1);
    for (uint32_t jj = 0; jj < nj; ++jj) {
      if (!v0[jj] || !v1[jj] || (g[jj] != 0 && (g[jj] & 1) == 0)) return hipErrorInvalidValue;
      a.v0[jj] = (const W*)v0[jj];
      a.v1[jj] = (const W*)v1[jj];
      a.g[jj] = (uint32_t)(g[jj] & (2 * N - 1));
      align |= ptr_bits(v0[jj], v1[jj]);
    }
    // workspace blocks alone: 16-byte accesses or nothing
    if (!vec_ok<W>(N, {}, align)) return hipErrorInvalidValue;
    const uint64_t bx = blocks_x<W>(limb_words, true);
    if (!grid_ok(bx, k.L)) return hipErrorInvalidConfiguration;
    const dim3 grid((unsigned)bx, (unsigned)k.L);
    with_bool(accum, [&](auto ACC) {
      hipLaunchKernelGGL((k_dh_bsgs_fold<W, decltype(ACC)::value>), grid, dim3(256), 0, k.s, (W*)A0, (W*)A1, a,
                         tab_ptrs<W>(k.t), k.t->log_n, limb_words, nj, limb_map(k));
    });
    return hipGetLastError();
  });
}

// The hybrid launchers: k.t the key basis' tables, k.L = Lv + K, k.B the
// chunk's polys.  The register tiers of alpha and K: 4, 8, 16, else the
// recomputing form (0).
hipError_t launch_modup(const Launch& k, void* D, const void* x, uint64_t src_ls, const HybridConsts& hc) {
  return by_word(k, [&](auto w) -> hipError_t {
    using W = decltype(w);
    const uint64_t N = 1ull << k.t->log_n;
    const uint64_t limb_words = (uint64_t)k.B * N;
    if (hc.alpha == 0 || hc.beta == 0 || hc.Lv == 0 || k.L != (size_t)hc.Lv + hc.K || !limb_map_ok(k) ||
        (uint64_t)hc.beta * hc.alpha < hc.Lv || (uint64_t)(hc.beta - 1) * hc.alpha >= hc.Lv || src_ls < limb_words)
      return hipErrorInvalidValue;
    if (limb_words == 0) return hipSuccess;
    // 16-byte accesses: whole vectors within a plane, every plane 16-byte aligned
    const bool vec = vec_ok<W>(N, {src_ls}, ptr_bits(D, x));
    const uint64_t bx = blocks_x<W>(limb_words, vec);
    if (!grid_ok(bx, hc.beta)) return hipErrorInvalidConfiguration;
    // runs of target limbs per lane: all of them in one lane where the vectors
    // alone fill the device (kSplitBlocks workgroups), else split over grid.z
    const LimbSplit sp = limb_split(k.L, bx * hc.beta);
    const dim3 grid((unsigned)bx, (unsigned)hc.beta, sp.extent);
    with_tier<4, 8, 16, 0>(hc.alpha, [&](auto AMAX) {
      with_bool(vec, [&](auto VEC) {
        hipLaunchKernelGGL((k_modup<W, decltype(VEC)::value, decltype(AMAX)::value>), grid, dim3(256), 0, k.s, (W*)D,
                           (const W*)x, tab_ptrs<W>(k.t), (const W*)hc.yinv, (const W*)hc.yinvp, (const W*)hc.conv,
                           (const W*)hc.convp, limb_words, src_ls, hc.alpha, hc.Lv, (uint32_t)k.L, sp.per,
                           limb_map(k));
      });
    });
    return hipGetLastError();
  });
}

hipError_t launch_moddown(const Launch& k, void* out, uint64_t out_ls, const void* A, uint64_t a_ls, const void* add,
                          uint64_t add_ls, const HybridConsts& hc) {
  return by_word(k, [&](auto w) -> hipError_t {
    using W = decltype(w);
    const uint64_t N = 1ull << k.t->log_n;
    const uint64_t limb_words = (uint64_t)k.B * N;
    if (hc.Lv == 0 || hc.K == 0 || k.L != (size_t)hc.Lv + hc.K || !limb_map_ok(k) || out_ls < limb_words ||
        a_ls < limb_words || (add && add_ls < limb_words))
      return hipErrorInvalidValue;
    if (limb_words == 0) return hipSuccess;
    const bool vec = vec_ok<W>(N, {out_ls, a_ls, add ? add_ls : 0}, ptr_bits(out, A, add));
    const uint64_t bx = blocks_x<W>(limb_words, vec);
    if (!grid_ok(bx)) return hipErrorInvalidConfiguration;
    const LimbSplit sp = limb_split(hc.Lv, bx);
    const dim3 grid((unsigned)bx, sp.extent);
    with_tier<4, 8, 16, 0>(hc.K, [&](auto KMAX) {
      with_bool(vec, [&](auto VEC) {
        hipLaunchKernelGGL((k_moddown<W, decltype(VEC)::value, decltype(KMAX)::value>), grid, dim3(256), 0, k.s,
                           (W*)out, out_ls, (const W*)A, a_ls, (const W*)add, add_ls, tab_ptrs<W>(k.t),
                           (const W*)hc.pinv, (const W*)hc.pinvp, (const W*)hc.pq, (const W*)hc.pqp, (const W*)hc.Pinv,
                           (const W*)hc.Pinvp, limb_words, hc.Lv, hc.K, sp.per, limb_map(k));
      });
    });
    return hipGetLastError();
  });
}

// The runs of the split are over the Lv - 1 output limbs.
hipError_t launch_moddown_rescale(const Launch& k, void* out, uint64_t out_ls, const void* A, uint64_t a_ls,
                                  const void* add, uint64_t add_ls, const void* rinv, const void* rinvp,
                                  const HybridConsts& hc, const MdAffine& af) {
  return by_word(k, [&](auto w) -> hipError_t {
    using W = decltype(w);
    const uint64_t N = 1ull << k.t->log_n;
    const uint64_t limb_words = (uint64_t)k.B * N;
    if (hc.Lv < 2 || hc.K == 0 || k.L != (size_t)hc.Lv + hc.K || !limb_map_ok(k) || out_ls < limb_words ||
        a_ls < limb_words || (add && add_ls < limb_words) || !rinv || !rinvp || (af.z && af.z_ls < limb_words))
      return hipErrorInvalidValue;
    if (limb_words == 0) return hipSuccess;
    const bool vec =
        vec_ok<W>(N, {out_ls, a_ls, add ? add_ls : 0, af.z ? af.z_ls : 0}, ptr_bits(out, A, add, af.z));
    const MdAffineArg<W> aa{(const W*)af.z, af.z_ls, af.w, af.u, af.bias, (uint32_t)(N - 1)};
    const uint64_t bx = blocks_x<W>(limb_words, vec);
    if (!grid_ok(bx)) return hipErrorInvalidConfiguration;
    const LimbSplit sp = limb_split(hc.Lv - 1, bx);
    const dim3 grid((unsigned)bx, sp.extent);
    with_tier<4, 8, 16, 0>(hc.K, [&](auto KMAX) {
      with_bool(vec, [&](auto VEC) {
        with_bool(af.on, [&](auto AFF) {
          hipLaunchKernelGGL(
              (k_moddown_rescale<W, decltype(VEC)::value, decltype(KMAX)::value, decltype(AFF)::value>), grid,
              dim3(256), 0, k.s, (W*)out, out_ls, (const W*)A, a_ls, (const W*)add, add_ls, tab_ptrs<W>(k.t),
              (const W*)hc.pinv, (const W*)hc.pinvp, (const W*)hc.pq, (const W*)hc.pqp, (const W*)hc.Pinv,
              (const W*)hc.Pinvp, (const W*)rinv, (const W*)rinvp, limb_words, hc.Lv, hc.K, sp.per, limb_map(k), aa);
        });
      });
    });
    return hipGetLastError();
  });
}

hipError_t launch_hoist_mac_seed(const Launch& k, void* acc0, void* acc1, const void* d, const void* key_a,
                                 const void* key_b, uint64_t key_ls, const void* seed_a, const void* seed_b,
                                 uint64_t seed_ls, const HybridConsts& hc) {
  return by_word(k, [&](auto w) -> hipError_t {
    using W = decltype(w);
    const uint64_t N = 1ull << k.t->log_n;
    const uint64_t limb_words = (uint64_t)k.B * N;
    const size_t Ls = k.src_limbs();
    if (Ls == 0 || key_ls < Ls * N || hc.Lv == 0 || k.L != (size_t)hc.Lv + hc.K || !limb_map_ok(k) ||
        seed_ls < limb_words || !seed_a || !seed_b || !hc.Pw || !hc.Pwp)
      return hipErrorInvalidValue;
    if (limb_words == 0) return hipSuccess;
    // 16-byte accesses: whole vectors within a plane, every plane and block 16-byte aligned
    const bool vec = vec_ok<W>(N, {key_ls, seed_ls}, ptr_bits(d, key_a, key_b, acc0, acc1, seed_a, seed_b));
    const uint64_t bx = blocks_x<W>(limb_words, vec);
    if (!grid_ok(bx, k.L)) return hipErrorInvalidConfiguration;
    const dim3 grid((unsigned)bx, (unsigned)k.L);
    with_bool(vec, [&](auto VEC) {
      hipLaunchKernelGGL((k_hoist_mac_seed<W, decltype(VEC)::value>), grid, dim3(256), 0, k.s, (W*)acc0, (W*)acc1,
                         (const W*)key_b, (const W*)key_a, (const W*)d, (const W*)seed_b, (const W*)seed_a, seed_ls,
                         (const W*)hc.Pw, (const W*)hc.Pwp, tab_ptrs<W>(k.t), k.t->log_n, limb_words, key_ls,
                         (uint32_t)Ls, hc.Lv, limb_map(k));
    });
    return hipGetLastError();
  });
}

// g odd, below 2N.  Grid x a multiple of 8 (xcd_gid()).
hipError_t launch_moddown_auto(const Launch& k, void* out, uint64_t out_ls, const void* A, uint64_t a_ls,
                               const void* add, uint64_t add_ls, uint64_t g, const HybridConsts& hc) {
  return by_word(k, [&](auto w) -> hipError_t {
    using W = decltype(w);
    const uint64_t N = 1ull << k.t->log_n;
    const uint64_t limb_words = (uint64_t)k.B * N;
    if (hc.Lv == 0 || hc.K == 0 || k.L != (size_t)hc.Lv + hc.K || !limb_map_ok(k) || out_ls < limb_words ||
        a_ls < limb_words || (add && add_ls < limb_words) || (g & 1) == 0 || g >= 2 * N)
      return hipErrorInvalidValue;
    if (limb_words == 0) return hipSuccess;
    // the stores are single words: only A and the addend decide the 16-byte
    // form, and the output need only be word-aligned
    const bool vec = vec_ok<W>(N, {a_ls, add ? add_ls : 0}, ptr_bits(A, add)) && (uintptr_t)out % sizeof(W) == 0;
    const uint64_t bx = blocks_x<W>(limb_words, vec, true);
    if (!grid_ok(bx)) return hipErrorInvalidConfiguration;
    const LimbSplit sp = limb_split(hc.Lv, bx);
    const dim3 grid((unsigned)bx, sp.extent);
    // (no 16-limb tier: with the destination offsets beside 16 z_k it spills
    // scalar registers; more than 8 special primes take the recomputing form)
    with_tier<4, 8, 0>(hc.K, [&](auto KMAX) {
      with_bool(vec, [&](auto VEC) {
        hipLaunchKernelGGL((k_moddown_auto<W, decltype(VEC)::value, decltype(KMAX)::value>), grid, dim3(256), 0, k.s,
                           (W*)out, out_ls, (const W*)A, a_ls, (const W*)add, add_ls, tab_ptrs<W>(k.t),
                           (const W*)hc.pinv, (const W*)hc.pinvp, (const W*)hc.pq, (const W*)hc.pqp, (const W*)hc.Pinv,
                           (const W*)hc.Pinvp, limb_words, k.t->log_n, (uint32_t)g, hc.Lv, hc.K, sp.per, limb_map(k));
      });
    });
    return hipGetLastError();
  });
}

// Clone: 4 x 16 B per lane, all four loads issued before the stores.
__global__ void __launch_bounds__(256)
k_copy16(uint4* __restrict__ dst, const uint4* __restrict__ src, uint64_t n16) {
  const uint64_t base = (uint64_t)blockIdx.x * 1024 + threadIdx.x;
  uint4 v[4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (base + u * 256 < n16) v[u] = src[base + u * 256];
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (base + u * 256 < n16) dst[base + u * 256] = v[u];
}

hipError_t launch_copy(hipStream_t s, void* dst, const void* src, uint64_t bytes) {
  const uint64_t n16 = bytes / 16;
  if (n16 == 0) return hipSuccess;
  const uint64_t blocks = (n16 + 1023) / 1024;
  if (blocks > 0x7fffffffull) return hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(k_copy16, dim3((unsigned)blocks), dim3(256), 0, s, (uint4*)dst,
                     (const uint4*)src, n16);
  return hipGetLastError();
}

// Strided copy: gridDim.y rows of `run` elements (16 bytes, or 4 where a
// pointer, a pitch or the run is not a multiple of 16), row r at + r pitch
// elements on either side -- polys [first, first + count) of every limb of a
// [L][B][N] buffer in one launch.
template <class E>
__global__ void __launch_bounds__(256)
k_copy_rows(E* __restrict__ dst, const E* __restrict__ src, uint64_t run, uint64_t dst_pitch,
            uint64_t src_pitch) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= run) return;
  dst[(uint64_t)blockIdx.y * dst_pitch + i] = src[(uint64_t)blockIdx.y * src_pitch + i];
}

hipError_t launch_copy_rows(hipStream_t s, void* dst, uint64_t dst_pitch_bytes, const void* src,
                            uint64_t src_pitch_bytes, uint64_t run_bytes, size_t rows) {
  if (run_bytes == 0 || rows == 0) return hipSuccess;
  if (rows > 65535 || dst_pitch_bytes < run_bytes || src_pitch_bytes < run_bytes) return hipErrorInvalidValue;
  const uint64_t all = (uint64_t)(uintptr_t)dst | (uint64_t)(uintptr_t)src | dst_pitch_bytes | src_pitch_bytes | run_bytes;
  if (all % 4 != 0) return hipErrorInvalidValue;  // (words are 4 or 8 bytes)
  const uint64_t eb = all % 16 == 0 ? 16 : 4;
  const uint64_t bx = (run_bytes / eb + 255) / 256;
  if (bx > 0x7fffffffull) return hipErrorInvalidConfiguration;
  const dim3 grid((unsigned)bx, (unsigned)rows);
  if (eb == 16)
    hipLaunchKernelGGL((k_copy_rows<uint4>), grid, dim3(256), 0, s, (uint4*)dst, (const uint4*)src, run_bytes / 16,
                       dst_pitch_bytes / 16, src_pitch_bytes / 16);
  else
    hipLaunchKernelGGL((k_copy_rows<uint32_t>), grid, dim3(256), 0, s, (uint32_t*)dst, (const uint32_t*)src,
                       run_bytes / 4, dst_pitch_bytes / 4, src_pitch_bytes / 4);
  return hipGetLastError();
}

// k.L = limbs of the INPUT; output has k.L - 1.
template <class W>
static hipError_t rescale_t(const Launch& k, void* out, const void* in) {
  const uint64_t pw = (uint64_t)k.B << k.t->log_n;
  const uint64_t total = pw * (k.L - 1);
  if (total == 0) return hipSuccess;
  const TabPtrs<W> tp = tab_ptrs<W>(k.t);
  const uint64_t last = k.L - 1;
  hipLaunchKernelGGL((k_rescale<W>), dim3(grid_for(pw, 256)), dim3(256), 0, k.s, (W*)out,
                     (const W*)in, (const W*)in + last * pw, tp.resc + last * tp.Lroot,
                     tp.rescp + last * tp.Lroot, tp, pw, pw, pw, (uint32_t)last);
  return hipGetLastError();
}

// rescale_t at limb strides of its own on either side (k.B polys per limb).
template <class W>
static hipError_t rescale_strided_t(const Launch& k, void* out, uint64_t out_ls, const void* in, uint64_t in_ls) {
  const uint64_t pw = (uint64_t)k.B << k.t->log_n;
  if (k.L == 0 || k.L > k.t->L || out_ls < pw || in_ls < pw) return hipErrorInvalidValue;
  if (pw * (k.L - 1) == 0) return hipSuccess;
  const TabPtrs<W> tp = tab_ptrs<W>(k.t);
  const uint64_t last = k.L - 1;
  hipLaunchKernelGGL((k_rescale<W>), dim3(grid_for(pw, 256)), dim3(256), 0, k.s, (W*)out,
                     (const W*)in, (const W*)in + last * in_ls, tp.resc + last * tp.Lroot,
                     tp.rescp + last * tp.Lroot, tp, in_ls, out_ls, pw, (uint32_t)last);
  return hipGetLastError();
}

// Rescale by a limb held outside the buffer (limb-sharded pipelines: the
// broadcast last limb of the global basis): out limbs 0..k.L-1 from in's.
template <class W>
static hipError_t rescale_ext_t(const Launch& k, void* out, const void* in, const void* lastp,
                                const void* inv, const void* invp) {
  const uint64_t pw = (uint64_t)k.B << k.t->log_n;
  const uint64_t total = pw * k.L;
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL((k_rescale<W>), dim3(grid_for(pw, 256)), dim3(256), 0, k.s, (W*)out,
                     (const W*)in, (const W*)lastp, (const W*)inv, (const W*)invp, tab_ptrs<W>(k.t),
                     pw, pw, pw, (uint32_t)k.L);
  return hipGetLastError();
}

// k.L = Lv limbs of the inputs, k.B = ciphertexts per term (rnt_internal.hpp).
// Register tiers: 4, 8 or 16 input vectors a lane; rescaling, 16 bytes of LDS a
// lane and output.
// The runs split the output limbs until the grid (two components) has
// kSplitBlocks workgroups.
hipError_t launch_lincomb(const Launch& k, void* out0, void* out1, uint64_t out_ls, const void* x0, const void* x1,
                          uint64_t in_ls, size_t n_in, size_t n_out, const void* w, const void* wp, const void* bias,
                          bool rescale) {
  return by_word(k, [&](auto word) -> hipError_t {
    using W = decltype(word);
    const uint64_t N = 1ull << k.t->log_n;
    const uint64_t ct_words = (uint64_t)k.B * N;
    if (n_in == 0 || n_in > kLincombMax || n_out == 0 || n_out > kLincombMax || k.L == 0 || k.L > k.t->L ||
        (rescale && k.L < 2) || in_ls < n_in * ct_words || out_ls < n_out * ct_words || !w || !wp || !out0 || !out1 ||
        !x0 || !x1)
      return hipErrorInvalidValue;
    if (ct_words == 0) return hipSuccess;
    // 16-byte accesses: whole vectors within a plane, every plane and term 16-byte aligned
    const bool vec = vec_ok<W>(N, {in_ls, out_ls}, ptr_bits(out0, out1, x0, x1));
    const uint64_t bx = blocks_x<W>(ct_words, vec);
    if (!grid_ok(bx)) return hipErrorInvalidConfiguration;
    const LimbSplit sp = limb_split(rescale ? k.L - 1 : k.L, 2 * bx);
    const dim3 grid((unsigned)bx, sp.extent, 2);
    const TabPtrs<W> tp = tab_ptrs<W>(k.t);
    const W* rinv = tp.resc + (k.L - 1) * tp.Lroot;
    const W* rinvp = tp.rescp + (k.L - 1) * tp.Lroot;
    const LincombGeom a{ct_words, in_ls, out_ls, (uint32_t)n_in, (uint32_t)n_out, (uint32_t)k.L, sp.per,
                        (uint32_t)(N - 1)};
    const size_t lds = rescale ? n_out * 256 * sizeof(uint4) : 0;  // (at most 64 KiB)
    with_tier<4, 8, 16>(n_in, [&](auto NI) {
      with_bool(vec, [&](auto VEC) {
        with_bool(rescale, [&](auto RESC) {
          hipLaunchKernelGGL((k_lincomb<W, decltype(VEC)::value, decltype(RESC)::value, decltype(NI)::value>), grid,
                             dim3(256), lds, k.s, (W*)out0, (W*)out1, (const W*)x0, (const W*)x1, (const W*)w,
                             (const W*)wp, (const W*)bias, rinv, rinvp, a, tp);
        });
      });
    });
    return hipGetLastError();
  });
}

// k.L = Lv limbs, k.B = the chunk's ciphertexts (rnt_internal.hpp).
hipError_t launch_dot_tensor(const Launch& k, void* d0, void* d1, void* d2, uint64_t out_ls, const void* x0,
                             const void* x1, const void* y0, const void* y1, uint64_t in_ls, uint64_t term_words,
                             size_t nt, bool accum) {
  return by_word(k, [&](auto w) -> hipError_t {
    using W = decltype(w);
    const uint64_t N = 1ull << k.t->log_n;
    const uint64_t limb_words = (uint64_t)k.B * N;
    if (nt == 0 || nt > kDotT || !limb_map_ok(k) || out_ls < limb_words || term_words < limb_words ||
        in_ls < (nt - 1) * term_words + limb_words || !d0 || !d1 || !d2 || !x0 || !x1 || !y0 || !y1)
      return hipErrorInvalidValue;
    if (limb_words == 0 || k.L == 0) return hipSuccess;
    // 16-byte accesses: whole vectors within a plane, every plane and term 16-byte aligned
    const bool vec = vec_ok<W>(N, {in_ls, out_ls, term_words}, ptr_bits(d0, d1, d2, x0, x1, y0, y1));
    const uint64_t bx = blocks_x<W>(limb_words, vec);
    if (!grid_ok(bx, k.L)) return hipErrorInvalidConfiguration;
    const dim3 grid((unsigned)bx, (unsigned)k.L);
    const DotGeom a{limb_words, term_words, in_ls, out_ls, (uint32_t)nt, accum ? 1u : 0u};
    with_bool(vec, [&](auto VEC) {
      with_bool(x0 == y0 && x1 == y1, [&](auto SQ) {
        hipLaunchKernelGGL((k_dot_tensor<W, decltype(VEC)::value, decltype(SQ)::value>), grid, dim3(256), 0, k.s,
                           (W*)d0, (W*)d1, (W*)d2, (const W*)x0, (const W*)x1, (const W*)y0, (const W*)y1, a,
                           tab_ptrs<W>(k.t), limb_map(k));
      });
    });
    return hipGetLastError();
  });
}

// k.L = Lv limbs, k.B = the chunk's ciphertexts (rnt_internal.hpp).
hipError_t launch_plain_mac(const Launch& k, void* d0, void* d1, uint64_t out_ls, const void* x0, const void* x1,
                            uint64_t in_ls, uint64_t term_words, const void* m, uint64_t m_ls, uint64_t m_term_words,
                            bool m_shared, const void* bias, uint64_t b_ls, bool b_shared, size_t nt, bool accum) {
  return by_word(k, [&](auto w) -> hipError_t {
    using W = decltype(w);
    const uint64_t N = 1ull << k.t->log_n;
    const uint64_t limb_words = (uint64_t)k.B * N;
    const uint64_t m_words = m_shared ? N : limb_words, b_words = b_shared ? N : limb_words;
    if (nt == 0 || nt > kPlainT || !limb_map_ok(k) || out_ls < limb_words || term_words < limb_words ||
        in_ls < (nt - 1) * term_words + limb_words || m_term_words < m_words ||
        m_ls < (nt - 1) * m_term_words + m_words || (bias && b_ls < b_words) || !d0 || !d1 || !x0 || !x1 || !m)
      return hipErrorInvalidValue;
    if (limb_words == 0 || k.L == 0) return hipSuccess;
    // 16-byte accesses: whole vectors within a plane, every plane and term 16-byte aligned -- the
    // plaintexts' and the bias' too
    const bool vec = vec_ok<W>(N, {in_ls, out_ls, term_words, m_ls, m_term_words, bias ? b_ls : 0},
                               ptr_bits(d0, d1, x0, x1, m, bias));
    const uint64_t bx = blocks_x<W>(limb_words, vec);
    if (!grid_ok(bx, k.L)) return hipErrorInvalidConfiguration;
    const dim3 grid((unsigned)bx, (unsigned)k.L);
    const PlainMacGeom a{limb_words, term_words, in_ls, out_ls, m_term_words, m_ls, m_shared ? N - 1 : ~0ull,
                         b_ls, b_shared ? N - 1 : ~0ull, (uint32_t)nt, accum ? 1u : 0u};
    with_bool(vec, [&](auto VEC) {
      hipLaunchKernelGGL((k_plain_mac<W, decltype(VEC)::value>), grid, dim3(256), 0, k.s, (W*)d0, (W*)d1,
                         (const W*)x0, (const W*)x1, (const W*)m, (const W*)bias, a, tab_ptrs<W>(k.t), limb_map(k));
    });
    return hipGetLastError();
  });
}

static uint64_t inv_mod_pow2(uint64_t h, uint64_t M) {
  // h odd, M power of two: Newton iteration for h^-1 mod 2^64, then mask.
  uint64_t x = h;  // correct to 3 bits
  for (int i = 0; i < 6; ++i) x *= 2 - h * x;
  return x & (M - 1);
}

template <class W>
static hipError_t automorphism_t(const Launch& k, void* out, const void* in, uint64_t g) {
  const uint64_t N = 1ull << k.t->log_n;
  const uint64_t two_n = 2 * N;
  const uint64_t e = g % two_n;
  const uint64_t pw = (uint64_t)k.B * N;
  const uint64_t total = pw * k.L;
  if (total == 0) return hipSuccess;
  if (k.L > 65535) return hipErrorInvalidConfiguration;
  const dim3 grid8((grid_for(pw, 256) + 7u) & ~7u, (unsigned)k.L);  // xcd_gid(): x a multiple of 8
  if (e & 1) {
    const uint64_t ginv = inv_mod_pow2(e, two_n);
    hipLaunchKernelGGL((k_automorph_odd<W>), grid8, dim3(256), 0, k.s,
                       (W*)out, (const W*)in, tab_ptrs<W>(k.t), k.t->log_n, ginv, pw, total);
  } else {
    uint32_t ex = 0;
    uint64_t h = e;
    while ((h & 1) == 0) {
      h >>= 1;
      ++ex;
    }
    const uint64_t M = two_n >> ex;
    const uint64_t hinv = inv_mod_pow2(h, M);
    hipLaunchKernelGGL((k_automorph_even<W>), grid8, dim3(256), 0, k.s,
                       (W*)out, (const W*)in, tab_ptrs<W>(k.t), k.t->log_n, ex, hinv, pw, total);
  }
  return hipGetLastError();
}

template <class W>
static hipError_t import_t(const Launch& k, void* dst, const uint64_t* stage, int to_brv,
                           unsigned long long* err) {
  const uint64_t total = ((uint64_t)k.B * k.L) << k.t->log_n;
  if (total == 0) return hipSuccess;
  const uint64_t ls = (uint64_t)k.B << k.t->log_n;
  hipLaunchKernelGGL((k_import<W>), dim3(grid_for(total, 256)), dim3(256), 0, k.s, (W*)dst,
                     stage, tab_ptrs<W>(k.t), k.t->log_n, (uint32_t)k.L, ls, to_brv, err, total);
  return hipGetLastError();
}

template <class W>
static hipError_t import_coeffs_t(const Launch& k, void* dst, const int64_t* stage) {
  const uint64_t total = (uint64_t)k.B << k.t->log_n;
  if (total == 0 || k.L == 0) return hipSuccess;
  hipLaunchKernelGGL((k_import_coeffs<W>), dim3(grid_for(total, 256)), dim3(256), 0, k.s,
                     (W*)dst, stage, tab_ptrs<W>(k.t), (uint32_t)k.L, total, total);
  return hipGetLastError();
}

template <class W>
static hipError_t export_t(const Launch& k, uint64_t* stage, const void* src, int from_brv,
                           uint64_t ls) {
  const uint64_t total = ((uint64_t)k.B * k.L) << k.t->log_n;
  if (total == 0) return hipSuccess;
  if (ls == 0) ls = (uint64_t)k.B << k.t->log_n;
  hipLaunchKernelGGL((k_export<W>), dim3(grid_for(total, 256)), dim3(256), 0, k.s, stage,
                     (const W*)src, k.t->log_n, (uint32_t)k.L, ls, from_brv, total);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// decode-side CRT (basis.rs:158-180, poly.rs:404-427)
// ---------------------------------------------------------------------------

// Per coefficient, with residues r_l (coefficient domain):
//   s_l = r_l * (Q/q_l)^-1 mod q_l,   x = sum_l s_l * (Q/q_l) - k * Q,
//   k = floor(sum_l s_l / q_l)  (double precision, then a +-Q correction),
// centred into (-Q/2, Q/2] and written as `out_words` little-endian 64-bit
// two's-complement words.  Multi-word values are MW 32-bit words; the
// constants (Q/q_l words, Q, floor(Q/2)) are wave-uniform scalar loads.
// (CrtConsts: rnt_internal.hpp)

template <int MW>
__device__ __forceinline__ bool mw_ge(const uint32_t (&a)[MW + 1], const RNT_CONST_AS uint32_t* b) {
  if (a[MW] != 0) return true;
#pragma unroll
  for (int w = MW - 1; w >= 0; --w) {
    if (a[w] != b[w]) return a[w] > b[w];
  }
  return true;
}
template <int MW>
__device__ __forceinline__ void mw_sub(uint32_t (&a)[MW + 1], const RNT_CONST_AS uint32_t* b) {
  uint64_t borrow = 0;
#pragma unroll
  for (int w = 0; w < MW; ++w) {
    const uint64_t d = (uint64_t)a[w] - b[w] - borrow;
    a[w] = (uint32_t)d;
    borrow = (d >> 32) & 1;
  }
  a[MW] -= (uint32_t)borrow;
}
template <int MW>
__device__ __forceinline__ void mw_add(uint32_t (&a)[MW + 1], const RNT_CONST_AS uint32_t* b) {
  uint64_t carry = 0;
#pragma unroll
  for (int w = 0; w < MW; ++w) {
    const uint64_t t = (uint64_t)a[w] + b[w] + carry;
    a[w] = (uint32_t)t;
    carry = t >> 32;
  }
  a[MW] += (uint32_t)carry;
}

template <class W, int MW>
__global__ void __launch_bounds__(256)
k_crt(uint64_t* __restrict__ out, const W* __restrict__ in, CrtConsts cc, TabPtrs<W> tp,
      uint32_t L, uint64_t ls, uint32_t out_words, uint64_t total) {
  const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= total) return;
  const RNT_CONST_AS uint32_t* qi = (const RNT_CONST_AS uint32_t*)cc.qi_words;
  const RNT_CONST_AS uint32_t* qw = (const RNT_CONST_AS uint32_t*)cc.q_words;
  const RNT_CONST_AS uint32_t* qh = (const RNT_CONST_AS uint32_t*)cc.qh_words;
  uint32_t acc[MW + 1];
#pragma unroll
  for (int w = 0; w <= MW; ++w) acc[w] = 0;
  double f = 0.0;
  for (uint32_t l = 0; l < L; ++l) {
    const LimbConst<W> lc = tp.lc[l];
    const W s = shoup_mul<W>(in[(uint64_t)l * ls + gid], (W)cc.inv[l], (W)cc.inv_p[l], lc.q);
    f += (double)s * cc.rq[l];
    // acc += s * (Q/q_l), s split into 32-bit halves
    const RNT_CONST_AS uint32_t* row = qi + (uint64_t)l * MW;
#pragma unroll
    for (int half = 0; half < (sizeof(W) == 8 ? 2 : 1); ++half) {
      const uint32_t sh = (uint32_t)((uint64_t)s >> (32 * half));
      uint64_t carry = 0;
#pragma unroll
      for (int w = 0; w + half < MW; ++w) {
        const uint64_t t = (uint64_t)sh * row[w] + acc[w + half] + carry;
        acc[w + half] = (uint32_t)t;
        carry = t >> 32;
      }
      // both halves stop at acc[MW - 1] (the high half has one product
      // fewer), so the carry out belongs in the top word either way
      acc[MW] += (uint32_t)carry;
    }
  }
  // subtract k*Q, k = floor(f) < L; then correct by at most one Q either way
  const uint32_t k = (uint32_t)f;
  {
    uint64_t borrow = 0;
    uint64_t carry = 0;
#pragma unroll
    for (int w = 0; w < MW; ++w) {
      const uint64_t kq = (uint64_t)k * qw[w] + carry;
      carry = kq >> 32;
      const uint64_t d = (uint64_t)acc[w] - (uint32_t)kq - borrow;
      acc[w] = (uint32_t)d;
      borrow = (d >> 32) & 1;
    }
    acc[MW] = acc[MW] - (uint32_t)carry - (uint32_t)borrow;
  }
  if ((int32_t)acc[MW] < 0) mw_add<MW>(acc, qw);
  if (mw_ge<MW>(acc, qw)) mw_sub<MW>(acc, qw);
  // centre: x > floor(Q/2)  <=>  x > Q/2 (Q odd)  ->  x - Q
  uint32_t t2[MW + 1];
#pragma unroll
  for (int w = 0; w <= MW; ++w) t2[w] = acc[w];
  bool gt = false;
  {
    bool decided = false;
#pragma unroll
    for (int w = MW - 1; w >= 0; --w) {
      if (!decided && t2[w] != qh[w]) {
        gt = t2[w] > qh[w];
        decided = true;
      }
    }
  }
  if (gt) mw_sub<MW>(acc, qw);  // negative: two's complement with sign in acc[MW]
  const uint32_t sign = (int32_t)acc[MW] < 0 ? 0xffffffffu : 0u;
  uint64_t* o = out + gid * out_words;
  for (uint32_t w = 0; w < out_words; ++w) {
    const uint32_t lo = 2 * w < (uint32_t)MW ? acc[2 * w] : sign;
    const uint32_t hi = 2 * w + 1 < (uint32_t)MW ? acc[2 * w + 1] : sign;
    o[w] = (uint64_t)lo | ((uint64_t)hi << 32);
  }
}

template <class W>
static hipError_t crt_t(const Launch& k, uint64_t* out, const void* in, const CrtConsts& cc,
                        uint32_t mw, uint32_t out_words) {
  const uint64_t total = (uint64_t)k.B << k.t->log_n;
  if (total == 0) return hipSuccess;
  const uint64_t ls = total;
#define RNT_L(MW)                                                                                \
  hipLaunchKernelGGL((k_crt<W, MW>), dim3(grid_for(total, 256)), dim3(256), 0, k.s, out,       \
                     (const W*)in, cc, tab_ptrs<W>(k.t), (uint32_t)k.L, ls, out_words, total); \
  return hipGetLastError()
  if (mw <= 4) { RNT_L(4); }
  if (mw <= 8) { RNT_L(8); }
  if (mw <= 16) { RNT_L(16); }
  if (mw <= 32) { RNT_L(32); }
  if (mw <= 64) { RNT_L(64); }
  if (mw <= 128) { RNT_L(128); }
#undef RNT_L
  return hipErrorInvalidValue;
}

hipError_t launch_rescale(const Launch& k, void* out, const void* in) {
  return by_word(k, [&](auto w) { return rescale_t<decltype(w)>(k, out, in); });
}
hipError_t launch_crt(const Launch& k, uint64_t* out, const void* in, const void* consts,
                      uint32_t mw, uint32_t out_words) {
  const CrtConsts cc = *(const CrtConsts*)consts;
  return by_word(k, [&](auto w) { return crt_t<decltype(w)>(k, out, in, cc, mw, out_words); });
}
hipError_t launch_rescale_ext(const Launch& k, void* out, const void* in, const void* last,
                              const void* inv, const void* invp) {
  return by_word(k, [&](auto w) { return rescale_ext_t<decltype(w)>(k, out, in, last, inv, invp); });
}
hipError_t launch_automorphism(const Launch& k, void* out, const void* in, uint64_t g) {
  return by_word(k, [&](auto w) { return automorphism_t<decltype(w)>(k, out, in, g); });
}
hipError_t launch_import(const Launch& k, void* dst, const uint64_t* stage, int to_brv,
                         unsigned long long* err) {
  return by_word(k, [&](auto w) { return import_t<decltype(w)>(k, dst, stage, to_brv, err); });
}
hipError_t launch_import_coeffs(const Launch& k, void* dst, const int64_t* stage) {
  return by_word(k, [&](auto w) { return import_coeffs_t<decltype(w)>(k, dst, stage); });
}
hipError_t launch_export(const Launch& k, uint64_t* stage, const void* src, int from_brv,
                         uint64_t ls) {
  return by_word(k, [&](auto w) { return export_t<decltype(w)>(k, stage, src, from_brv, ls); });
}
hipError_t launch_rescale_strided(const Launch& k, void* out, uint64_t out_ls, const void* in, uint64_t in_ls) {
  return by_word(k, [&](auto w) { return rescale_strided_t<decltype(w)>(k, out, out_ls, in, in_ls); });
}
hipError_t launch_mont_one(const Launch& k, void* out) {
  return by_word(k, [&](auto w) { return mont_one_t<decltype(w)>(k, out); });
}
}  // namespace rnt
