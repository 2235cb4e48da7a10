// rnt_raise.hip -- the two streaming kernels on either side of the
// coefficient/slot transforms (DESIGN.md §4 "ModRaise and the coefficient/slot
// transforms"):
//
//   k_mod_raise     rnt_mod_raise: the centred CRT value of l0 <= 4 limbs
//                   reduced into every limb of a longer basis
//   k_mul_monomial  rnt_mul_monomial: out = in X^k in Z_q[X]/(X^N + 1), a
//                   negacyclic shift
//
// Both read and write [limb][poly][N] planes; a lane owns 16 bytes of a plane
// where every plane is 16-byte aligned (VEC) and one word otherwise, so every
// store is a full coalesced vector store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rnt_device.hpp"
#include "rnt_internal.hpp"
#include "rnt_launch.hpp"
#include "rnt_modarith.hpp"

namespace rnt {

namespace {

// ModRaise.  A lane reads its vector of the L0 input planes once and forms
// the mixed-radix digits d_0 .. d_{L0-1} of x in [0, Q0) -- x = d_0 + q_0 d_1 +
// q_0 q_1 d_2 + ..., d_i < q_i -- with word arithmetic alone (d_k < q_k may
// exceed q_i: the Shoup product takes any word).  x > floor(Q0 / 2) is the
// lexicographic comparison of the digits with those of floor(Q0 / 2), from the
// top.  Limbs j < L0 of the output are the input's words; limb j >= L0 is
//   sum_i d_i rad[j][i] - [x > floor(Q0/2)] q0m[j]  mod q_j,
// rad[j][i] = q_0 .. q_{i-1} mod q_j and q0m[j] = Q0 mod q_j (device arrays
// over the root limbs of the output's tables tp).  blockIdx.y takes a run of
// jper output limbs, so that one ciphertext's vectors still fill the device.
template <class W, bool VEC, int L0>
__global__ void __launch_bounds__(256)
k_mod_raise(W* __restrict__ out, uint64_t out_ls, const W* __restrict__ in, uint64_t in_ls, TabPtrs<W> tp,
            const W* __restrict__ rad, const W* __restrict__ radp, const W* __restrict__ q0m, RaiseDigits g,
            uint64_t limb_words, uint32_t L, uint32_t jper) {
  constexpr int V = VEC ? 16 / (int)sizeof(W) : 1;
  const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (i >= limb_words) return;
  const uint32_t j0 = blockIdx.y * jper;
  const uint32_t j1 = j0 + jper < L ? j0 + jper : L;
  W x[L0][V], d[L0][V];
  bool neg[V];
#pragma unroll
  for (int a = 0; a < L0; ++a) ld_vec<W, VEC, V>(x[a], in + (uint64_t)a * in_ls + i);
#pragma unroll
  for (int v = 0; v < V; ++v) d[0][v] = x[0][v];
#pragma unroll
  for (int a = 1; a < L0; ++a) {
    const W q = tp.lc[a].q;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      W s = (W)0;
#pragma unroll
      for (int k = 0; k < a; ++k) s = add_mod<W>(s, shoup_mul<W>(d[k][v], (W)g.pre[a][k], (W)g.prep[a][k], q), q);
      d[a][v] = shoup_mul<W>(x[a][v] - s + q, (W)g.ginv[a], (W)g.ginvp[a], q);  // x - s + q in (0, 2q)
    }
  }
#pragma unroll
  for (int v = 0; v < V; ++v) {
    bool gt = false, eq = true;
#pragma unroll
    for (int a = L0 - 1; a >= 0; --a) {
      const W h = (W)g.half[a];
      gt = gt || (eq && d[a][v] > h);
      eq = eq && d[a][v] == h;
    }
    neg[v] = gt;
  }
  for (uint32_t j = j0; j < j1; ++j) {
    W r[V];
    if (j < (uint32_t)L0) {  // (uniform) the input's own limb
#pragma unroll
      for (int a = 0; a < L0; ++a)
        if ((uint32_t)a == j) {
#pragma unroll
          for (int v = 0; v < V; ++v) r[v] = x[a][v];
        }
    } else {
      const W q = tp.lc[j].q, c = q0m[j];
#pragma unroll
      for (int v = 0; v < V; ++v) r[v] = (W)0;
#pragma unroll
      for (int a = 0; a < L0; ++a) {
        const W w = rad[(uint64_t)j * kRaiseMax + a], wp = radp[(uint64_t)j * kRaiseMax + a];
#pragma unroll
        for (int v = 0; v < V; ++v) r[v] = add_mod<W>(r[v], shoup_mul<W>(d[a][v], w, wp, q), q);
      }
#pragma unroll
      for (int v = 0; v < V; ++v) r[v] = sub_mod<W>(r[v], neg[v] ? c : (W)0, q);
    }
    st_vec<W, VEC, V>(out + (uint64_t)j * out_ls + i, r);
  }
}

// out = in X^k, k in [0, 2N): output word t of a poly is input word (t - k)
// mod 2N when that is below N, else the negated word (t - k) mod 2N - N.  A
// lane owns V consecutive outputs; its sources are consecutive too up to the
// wrap, so with k a multiple of V (every plane 16-byte aligned) the load is
// one vector as well (ALN); else V word loads from one or two cache lines.
template <class W, bool VEC, bool ALN>
__global__ void __launch_bounds__(256)
k_mul_monomial(W* __restrict__ out, const W* __restrict__ in, TabPtrs<W> tp, uint32_t log_n, uint32_t k,
               uint64_t limb_words) {
  constexpr int V = VEC ? 16 / (int)sizeof(W) : 1;
  const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (i >= limb_words) return;
  const uint32_t l = blockIdx.y;
  const uint32_t N = 1u << log_n, m2 = 2 * N - 1;
  const W q = tp.lc[l].q;
  const uint32_t t = (uint32_t)i & (N - 1);
  const uint64_t base = (uint64_t)l * limb_words + (i - t);  // word 0 of the lane's poly
  W r[V];
  if constexpr (VEC && ALN) {
    const uint32_t s = (t - k) & m2;  // a multiple of V: the V sources do not wrap
    ld_vec<W, true, V>(r, in + base + (s & (N - 1)));
    if (s >= N) {
#pragma unroll
      for (int v = 0; v < V; ++v) r[v] = r[v] == 0 ? (W)0 : (W)(q - r[v]);
    }
  } else {
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const uint32_t s = (t + (uint32_t)v - k) & m2;
      const W c = in[base + (s & (N - 1))];
      r[v] = s < N ? c : (c == 0 ? (W)0 : (W)(q - c));
    }
  }
  st_vec<W, VEC, V>(out + (uint64_t)l * limb_words + i, r);
}

}  // namespace

// The output limbs are split over blockIdx.y below kSplitBlocks workgroups (as
// the hybrid kernels'); one instantiation per input limb count l0 <= kRaiseMax.
hipError_t launch_mod_raise(const Launch& k, void* out, const void* in, size_t l0, const RaiseConsts& rc) {
  return by_word(k, [&](auto w) -> hipError_t {
    using W = decltype(w);
    const uint64_t N = 1ull << k.t->log_n;
    const uint64_t limb_words = (uint64_t)k.B * N;
    if (l0 == 0 || l0 > kRaiseMax || l0 >= k.L || k.L > k.t->L || !out || !in || !rc.rad || !rc.radp || !rc.q0m)
      return hipErrorInvalidValue;
    if (limb_words == 0) return hipSuccess;
    // 16-byte accesses: whole vectors within a plane, every plane 16-byte aligned
    const bool vec = vec_ok<W>(N, {}, ptr_bits(out, in));
    const uint64_t bx = blocks_x<W>(limb_words, vec);
    if (!grid_ok(bx)) return hipErrorInvalidConfiguration;
    const LimbSplit sp = limb_split(k.L, bx);
    const dim3 grid((unsigned)bx, sp.extent);
    with_tier<1, 2, 3, 4>(l0, [&](auto L0) {
      with_bool(vec, [&](auto VEC) {
        hipLaunchKernelGGL((k_mod_raise<W, decltype(VEC)::value, decltype(L0)::value>), grid, dim3(256), 0, k.s,
                           (W*)out, limb_words, (const W*)in, limb_words, tab_ptrs<W>(k.t), (const W*)rc.rad,
                           (const W*)rc.radp, (const W*)rc.q0m, rc.g, limb_words, (uint32_t)k.L, sp.per);
      });
    });
    return hipGetLastError();
  });
}

hipError_t launch_mul_monomial(const Launch& k, void* out, const void* in, uint64_t shift) {
  return by_word(k, [&](auto w) -> hipError_t {
    using W = decltype(w);
    const uint64_t N = 1ull << k.t->log_n;
    const uint64_t limb_words = (uint64_t)k.B * N;
    if (shift >= 2 * N || !out || !in || out == in) return hipErrorInvalidValue;
    if (limb_words == 0 || k.L == 0) return hipSuccess;
    const bool vec = vec_ok<W>(N, {}, ptr_bits(out, in));
    const uint64_t bx = blocks_x<W>(limb_words, vec);
    if (!grid_ok(bx, k.L)) return hipErrorInvalidConfiguration;
    const dim3 grid((unsigned)bx, (unsigned)k.L);
    // ALN: the shift a whole number of vectors too (VEC alone else; never ALN without VEC)
    with_bool(vec, [&](auto VEC) {
      with_bool(vec && shift % (16 / sizeof(W)) == 0, [&](auto ALN) {
        if constexpr (decltype(VEC)::value || !decltype(ALN)::value)
          hipLaunchKernelGGL((k_mul_monomial<W, decltype(VEC)::value, decltype(ALN)::value>), grid, dim3(256), 0, k.s,
                             (W*)out, (const W*)in, tab_ptrs<W>(k.t), k.t->log_n, (uint32_t)shift, limb_words);
      });
    });
    return hipGetLastError();
  });
}

}  // namespace rnt
