// rnt_rows.hip -- the kernels on the row passes of the four-step transform
// (rnt_fourstep.hpp) and their launchers:
//   k_row                  forward / inverse rows in place and the poly-mul rows
//                          (MulAssign, poly.rs:277-331), as rows of a plane or
//                          (WHOLE) as the whole plane in one launch
//   k_ks_rows, k_ks_whole  the gadget key-switch sum
//   k_tensor_rows          the ciphertext tensor product
// One unit on purpose: the three families instantiate the same pass templates
// (xf_fwd / xf_inv / xchg over RowGeo<LOG_C>), and the compiler's code for a
// kernel depends on which other users of those templates share its module --
// compiled apart, 38 of their kernels come out scheduled differently, some
// with other register and spill counts (profiles/split_kernels_device_code.txt).
#include <hip/hip_runtime.h>

#include "rnt_fourstep.hpp"
#include "rnt_launch.hpp"

namespace rnt {

// ---------------------------------------------------------------------------
// row passes and whole-plane products: k_row
// ---------------------------------------------------------------------------

// ---- the truncated product (rnt_mul's row kernel, u32 canonical bases) ----
// The forward transforms stop two stages early: block b of 4 consecutive
// device-order words then holds the residue of the operand mod X^4 - zeta_b,
// zeta_b = psi_rev[N/4 + b]^2 = (-1)^b psi_rev[N/8 + b/2] (the heap's
// children square to their parent's root, and the odd child carries -1).
// The product of two such residues is a degree-3 negacyclic-style product;
// the inverse transforms skip the same two stages, and the inverse column
// pass folds 4/N instead of 1/N (LimbConst c1t/c2t).  Exact arithmetic, so
// the coefficient-domain result is bit-identical to the full transform's.
template <int LOG_C>
struct Trunc {
  static constexpr bool on = LOG_C >= 4 && LOG_C % 4 == 0;  // last row pass = a whole radix-16 pass
};
template <class W, int LOG_C, bool LZ>
constexpr bool trunc_mul() {
  return sizeof(W) == 4 && !LZ && Trunc<LOG_C>::on;
}

// rnt_mul runs the Harvey-lazy kernels exactly when lazy_ok(); otherwise
// its u32 row kernel truncates when the row length allows (Trunc<LOG_C>).
bool mul_truncated(const Tables* t) {
  if (t->wide || lazy_ok(t)) return false;
  const Geom g = geom_for(t->log_n);
  return g.log_c >= 4 && g.log_c % 4 == 0;
}

// mode 0: forward rows in place; 1: inverse rows in place;
// 2: poly-mul rows: out <- INV(FWD(x) (.) FWD(y)) with Montgomery pointwise
// (out = x in the four-step product).
// WHOLE (log_n = LOG_C <= 14): a row is the whole plane (R = 1), so the
// transforms are the whole network and the inverse's top stage applies the
// folded n^-1 constants (with the Montgomery factor after a product, 4/N
// after a truncated one) that the inverse column pass applies otherwise:
// the product is one launch moving 3 planes per (poly, limb), a transform
// one launch moving 2.
// Minimum waves per SIMD of the u64 lazy (q < 2^62) product rows: 3 lets
// them take up to 168 VGPRs; at 4 (128 VGPRs, 60 bytes a lane of spills at
// 2^8-word rows) 2^16 x 16 x 62-bit ran 1.6% slower (41.10k against 41.75k
// poly-muls/s, row kernel 2.99 against 2.92 ms, profiles/r06/ab_u64_waves.txt)
#ifndef RNT_U64_LZ_WAVES
#define RNT_U64_LZ_WAVES 3
#endif
// RNT_U64_WHOLE_WAVES / RNT_U64_WHOLE_LZ: the u64 whole-plane product's
// occupancy bound (4: two 512-thread workgroups a CU at 128 VGPRs; 2: one
// at 256) and its arithmetic (1: Harvey-lazy where every q < 2^62)
#ifndef RNT_U64_WHOLE_WAVES
#define RNT_U64_WHOLE_WAVES 4
#endif
#ifndef RNT_U64_WHOLE_LZ
#define RNT_U64_WHOLE_LZ 0
#endif
template <class W, int MODE, int LOG_C, bool LZ = false, bool WHOLE = false>
__global__ void __launch_bounds__(RowGeo<LOG_C>::THREADS, sizeof(W) == 4 ? (WHOLE ? kWholeMinWaves : kRowMinWaves)
                                                                 : (MODE == 2 && LOG_C >= (WHOLE ? 13 : 7)
                                                                        ? (LZ && !WHOLE ? RNT_U64_LZ_WAVES
                                                                                        : WHOLE ? RNT_U64_WHOLE_WAVES : 4)
                                                                        : 1))
k_row(W* __restrict__ xg, const W* __restrict__ yg, W* __restrict__ outg, TabPtrs<W> tp, uint32_t log_n,
      uint32_t B, uint64_t ls, uint64_t rows_total) {
  using G = RowGeo<LOG_C>;
  constexpr int E = G::E;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  W* lds = (W*)smem_raw;
  // poly index fastest: a workgroup's rows share (limb, row r) and with it
  // every twiddle, which then comes from L1 (profiles/r02_ab_row_pfast.txt)
  const RowPos rp = row_pos_pfast<G>(log_n, B, rows_total);
  const uint64_t N = 1ull << log_n;
  const uint64_t base = (uint64_t)rp.l * ls + (uint64_t)rp.p * N + (uint64_t)rp.r * G::C;
  const LimbConst<W> lc = tp.lc[rp.l];
  const Tw<W>* tw = tp.tw + (uint64_t)rp.l * N;
  const Tw<W>* itw = tp.itw + (uint64_t)rp.l * N;
  const uint32_t b0 = G::base(rp.xp.tau, G::BB0);
  const uint32_t bl = G::base(rp.xp.tau, G::BBL);
  if constexpr (MODE == 2) {
    W v[2][E];
#pragma unroll
    for (int i = 0; i < E; ++i) {
      v[0][i] = gload(xg, base + b0 + ((uint32_t)i << G::BB0));
      v[1][i] = gload(yg, base + b0 + ((uint32_t)i << G::BB0));
    }
    const auto mo = mod_for<W, LZ>(lc);
    // the product overwrites operand 0's registers (z aliases v[0]): the
    // inverse then holds one plane, not three
    W (&z)[1][E] = *reinterpret_cast<W(*)[1][E]>(&v[0]);
    if constexpr (trunc_mul<W, LOG_C, LZ>()) {
      // every pass but the last in full, the last without its two stages
      if constexpr (G::P > 1) fwd_pass<G, W, 2, 0>(v, rp.xp, lds, tw, mo);
      if constexpr (G::P > 2) fwd_pass<G, W, 2, 1>(v, rp.xp, lds, tw, mo);
      if constexpr (G::P > 3) fwd_pass<G, W, 2, 2>(v, rp.xp, lds, tw, mo);
      fwd_pass<G, W, 2, G::P - 1, 2>(v, rp.xp, lds, tw, mo);
      // blocks t of 4 registers: device positions r*C + tau*E + 4t (G::BBL == 0)
      static_assert(G::BBL == 0 && E == 16, "truncated product layout");
      const uint32_t zb = (uint32_t)(N >> 3) + ((rp.r * (uint32_t)G::C) >> 3) + (rp.xp.tau << 1);
      const Tw<W> zw[2] = {tw[zb], tw[zb + 1]};
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const Tw<W> w = zw[t >> 1];
        const uint32_t zeta = (t & 1) ? (uint32_t)lc.q - w.w : w.w;  // (-1)^b psi_rev[N/8 + b/2]
        const uint32_t zeta_p = (t & 1) ? ~w.p : w.p;                  // Shoup companion of q - w
        uint32_t c[4];
        mul_mod_x4(c, &v[0][4 * t], &v[1][4 * t], zeta, zeta_p, lc.q, lc.qinv);
#pragma unroll
        for (int k = 0; k < 4; ++k) z[0][4 * t + k] = c[k];
      }
      const Fold<W> ft = WHOLE ? Fold<W>{lc.c1t, lc.c1t_p, lc.c2t, lc.c2t_p} : Fold<W>{};
      inv_pass<G, W, 1, G::P - 1, WHOLE, 2>(z, rp.xp, lds, itw, mo, ft);
      if constexpr (G::P > 3) inv_pass<G, W, 1, 2, WHOLE>(z, rp.xp, lds, itw, mo, ft);
      if constexpr (G::P > 2) inv_pass<G, W, 1, 1, WHOLE>(z, rp.xp, lds, itw, mo, ft);
      if constexpr (G::P > 1) inv_pass<G, W, 1, 0, WHOLE>(z, rp.xp, lds, itw, mo, ft);
    } else {
    xf_fwd<G, W, 2>(v, rp.xp, lds, tw, mo);
    if constexpr (LZ && sizeof(W) == 4) {
      // [0, 4q) inputs -> [0, 2q); a b < 4q^2 < q 2^32, so the Montgomery
      // quotient leaves (ab + mq) / 2^32 < 2q: the GS passes' input range
#pragma unroll
      for (int i = 0; i < E; ++i) {
        const uint32_t a = csub<uint32_t>(v[0][i], mo.q2), b = csub<uint32_t>(v[1][i], mo.q2);
        const uint64_t t = mul64(a, b);
        const uint32_t mm = (uint32_t)t * (0u - (uint32_t)lc.qinv);
        z[0][i] = (uint32_t)(mad64(mm, (uint32_t)lc.q, t) >> 32);
      }
    } else if constexpr (LZ) {
      // u64, q < 2^62: [0, 4q) -> [0, 2q) inputs; hi(a b) < 4q^2 / 2^64 < q
      // and hi(m q) < q, so mont_mul's final sub_mod gives the canonical
      // product (the GS passes take [0, 2q))
#pragma unroll
      for (int i = 0; i < E; ++i)
        z[0][i] = mont_mul<W>(csub<W>(v[0][i], mo.q2), csub<W>(v[1][i], mo.q2), lc.q, lc.qinv);
    } else {
#pragma unroll
      for (int i = 0; i < E; ++i) z[0][i] = mont_mul<W>(v[0][i], v[1][i], lc.q, lc.qinv);
    }
    xf_inv<G, W, 1, WHOLE>(z, rp.xp, lds, itw, mo,
                           WHOLE ? Fold<W>{lc.c1r, lc.c1r_p, lc.c2r, lc.c2r_p} : Fold<W>{});
    }
    if (rp.active) {
#pragma unroll
      for (int i = 0; i < E; ++i) gstore(outg, base + b0 + ((uint32_t)i << G::BB0), z[0][i]);
    }
  } else if constexpr (MODE == 0) {
    W v[1][E];
#pragma unroll
    for (int i = 0; i < E; ++i) v[0][i] = xg[base + b0 + ((uint32_t)i << G::BB0)];
    xf_fwd<G, W, 1>(v, rp.xp, lds, tw, mod_of(lc));
    if (rp.active) {
#pragma unroll
      for (int i = 0; i < E; ++i) xg[base + bl + ((uint32_t)i << G::BBL)] = v[0][i];
    }
  } else {
    W v[1][E];
#pragma unroll
    for (int i = 0; i < E; ++i) v[0][i] = xg[base + bl + ((uint32_t)i << G::BBL)];
    xf_inv<G, W, 1, WHOLE>(v, rp.xp, lds, itw, mod_of(lc),
                           WHOLE ? Fold<W>{lc.c1, lc.c1_p, lc.c2, lc.c2_p} : Fold<W>{});
    if (rp.active) {
#pragma unroll
      for (int i = 0; i < E; ++i) xg[base + b0 + ((uint32_t)i << G::BB0)] = v[0][i];
    }
  }
}

template <class W, int MODE, int LOG_C, bool LZ = false, bool WHOLE = false>
static hipError_t row_launch(const Launch& k, void* x, const void* y, uint64_t ls, void* out = nullptr) {
  using G = RowGeo<LOG_C>;
  const Geom g = geom_for(k.t->log_n);
  const uint64_t rows = (uint64_t)k.L * k.B * (WHOLE ? 1 : g.r);
  if (rows == 0) return hipSuccess;
  const uint64_t blocks = (rows + G::RPW - 1) / G::RPW;
  if (blocks > 0x7fffffffull) return hipErrorInvalidConfiguration;
  const size_t lds = row_lds<W, LOG_C>(MODE == 2 ? 2 : 1);
  hipError_t e = allow_lds(k_row<W, MODE, LOG_C, LZ, WHOLE>, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_row<W, MODE, LOG_C, LZ, WHOLE>), dim3((unsigned)blocks), dim3(G::THREADS), lds, k.s,
                     (W*)x, (const W*)y, (W*)(out ? out : x), tab_ptrs<W>(k.t, k.tab0), WHOLE ? (uint32_t)LOG_C : g.log_n,
                     (uint32_t)k.B, ls, rows);
  return hipGetLastError();
}

// The whole-plane row path (k_row<..., WHOLE>): every (poly, limb) plane is
// one row.  u32 and u64 words at 2^10 <= N <= 2^14 (a row of 2^14 words is
// 1024 threads x 16 registers); RNT_PLANE=0 keeps the four-step kernels.
// The u64 four-step product rows of 2^7..2^9 words are capped at 128 VGPRs
// too (they took 131-132, three waves per SIMD; 12-28 bytes of spills):
// k_row<2> at 2^16 x 16 x 62-bit 3.03-3.09 against 3.17-3.23 ms per 256
// pairs (profiles/r04/ab_u64_rows.txt).
// The u64 product rows at 2^13 and 2^14 are capped at 128 VGPRs (four
// waves per SIMD: 2^13 spills 92 bytes a lane, 2^14 12): uncapped they
// took ~150 and a CU held one workgroup (2^13 x 7 x 61-bit: 0.67M against
// the four-step kernels' 0.76M poly-muls/s); capped, 0.80M against 0.75M
// at 2^13 x 7 and 0.80M against 0.795M at 2^14 x 3, same box
// (profiles/r04/ab_u64_whole.txt).
bool whole_ok(const Tables* t, int mode) {
  (void)mode;
  return t->plane != 0 && t->log_n >= 10 && t->log_n <= 14;
}

template <class W>
static hipError_t whole_t(const Launch& k, int mode, void* out, void* x, const void* y, uint64_t ls, bool lz) {
#define RNT_W(C)                                                                                      \
  case C:                                                                                             \
    if (mode == 0) return row_launch<W, 0, C, false, true>(k, x, nullptr, ls);                        \
    if (mode == 1) return row_launch<W, 1, C, false, true>(k, x, nullptr, ls);                        \
    if (lz) return row_launch<W, 2, C, true, true>(k, x, y, ls, out);                                 \
    return row_launch<W, 2, C, false, true>(k, x, y, ls, out);
  switch (k.t->log_n) {
    RNT_W(10)
    RNT_W(11)
    RNT_W(12)
    RNT_W(13)
    RNT_W(14)
    default: return hipErrorInvalidValue;
  }
#undef RNT_W
}

template <class W>
static hipError_t row_t(const Launch& k, int mode, void* x, const void* y, uint64_t ls, bool lz) {
  const Geom g = geom_for(k.t->log_n);
#define RNT_L0(C) return row_launch<W, 0, C>(k, x, y, ls)
#define RNT_L1(C) return row_launch<W, 1, C>(k, x, y, ls)
#define RNT_L2(C) return row_launch<W, 2, C>(k, x, y, ls)
#define RNT_L2Z(C) return row_launch<W, 2, C, true>(k, x, y, ls)
  if (mode == 2 && lz) {
    RNT_DISPATCH_LOGC(g.log_c, RNT_L2Z)
  }
  if (mode == 0) {
    RNT_DISPATCH_LOGC(g.log_c, RNT_L0)
  } else if (mode == 1) {
    RNT_DISPATCH_LOGC(g.log_c, RNT_L1)
  } else {
    RNT_DISPATCH_LOGC(g.log_c, RNT_L2)
  }
#undef RNT_L0
#undef RNT_L1
#undef RNT_L2
#undef RNT_L2Z
  return hipErrorInvalidValue;
}

hipError_t launch_row(const Launch& k, int mode, void* x, const void* y, uint64_t ls, bool lazy) {
  const bool lz = lazy && lazy_ok(k.t);
  return by_word(k, [&](auto w) { return row_t<decltype(w)>(k, mode, x, y, ls, lz); });
}
hipError_t launch_whole(const Launch& k, int mode, void* out, void* x, const void* y, uint64_t ls) {
  // the Harvey-lazy arithmetic where every modulus < 2^30 (u32 words), as
  // rnt_mul's four-step path.  The u64 whole-plane product stays canonical:
  // capped at 128 VGPRs its lazy form spills 240 bytes a lane at 2^13 (92
  // canonical) and measured 6.3% slower at the horner_chain.rs shape,
  // 2^13 x 7 x 61-bit (0.792M against 0.845M poly-muls/s, same box,
  // profiles/r06/ab_lazy62.txt); the u64 four-step product takes it (+7.9%)
  const bool lz = k.t->wide ? (RNT_U64_WHOLE_LZ && k.t->lazy62 != 0) : k.t->lazy30 != 0;
  return by_word(k, [&](auto w) { return whole_t<decltype(w)>(k, mode, out, x, y, ls, lz); });
}

// ---------------------------------------------------------------------------
// the gadget key-switch sum (engine.rs:505-528, 429-452): k_ks_rows, k_ks_whole
// ---------------------------------------------------------------------------

// Words per padded LDS key row: C + C/16 (ks_pad's 4 per 64), rounded up to
// a whole 16-byte unit (the host sizes the LDS with the same formula).
template <class W>
__host__ __device__ constexpr int ks_kpad_words(int c) {
  constexpr int V = 16 / (int)sizeof(W);
  return (c + (c >> 4) + V - 1) / V * V;
}
// Padded LDS position of key word w: 4 pad words per 64, so the 16-byte
// reads of 16 lanes at 64-byte strides (a row's E = 16 consecutive words per
// thread) start on 16 distinct 4-bank groups, and 16-byte alignment holds.
__device__ __forceinline__ uint32_t ks_pad(uint32_t w) { return w + ((w >> 6) << 2); }
// LDS plan of k_ks_rows<W, LOG_C, NP>, shared by the kernel and its launcher.
//  * KEYGLDS: u32 rows of >= 64 words take the key rows global -> LDS
//    directly (global_load_lds);
//  * KDOUBLE: two key buffers (the next limb's keys are written while the
//    last ones may still be read) when they fit beside the exchange region in
//    a quarter of the LDS, else one buffer and a barrier per limb.
// (Staging the next source limb's S rows global -> LDS one limb ahead
// measured slower, ks_rows 2.40 against 2.31 ms per 64-ct chunk,
// profiles/r03/ab_ks_spre.txt, as register prefetch of the next limb did
// before it: the rows kernel does not wait on the S loads.)
//  * KSPLIT: when even one {key_b, key_a} buffer would push the workgroup
//    past a quarter of the LDS (the one-poly grid, NP = 1: 8 or 16 rows of
//    both keys beside the exchange region, 52 KiB), key_a's rows go into
//    the exchange region once the transform's last exchange is done, so
//    four workgroups fit a CU (three left a 1024-workgroup grid 1.33
//    rounds long).
//  * KREG: the one-poly grid (NP = 1) of u32 rows of >= 64 words shares no
//    key word between threads, so each thread loads its own E words of both
//    keys straight into registers, issued with the S row and landing while
//    the row transform runs; no key LDS, no key barriers.  With KSPLIT the
//    one-ciphertext rotation waited twice a source limb (S + key_b, then
//    key_a after the transform).  RNT_KS_SPRE: the S row of the next source
//    limb also loads one limb ahead (16 registers).  Off: parity-green, but
//    the 32 key registers live across the transform spill (176 bytes a lane
//    without SPRE, 352 with it, against 104) and the rows kernel measured
//    0.4749 / 0.6573 ms against 0.4513 ms a one-ciphertext rotation at config
//    5 (profiles/r06/ab_ks_kreg.txt); with the loads after the transform
//    (RNT_KS_KLATE) hipcc still spills 272 bytes.
#ifndef RNT_KS_KREG
#define RNT_KS_KREG 0
#endif
#ifndef RNT_KS_SPRE
#define RNT_KS_SPRE 1
#endif
#ifndef RNT_KS_KLATE
#define RNT_KS_KLATE 0
#endif
// RNT_KS_KREG_WAVES: the KREG grid's occupancy bound (workgroups a CU the
// launch bounds promise): 2 gives its registers room (256 VGPRs: the keys and
// the next S row in flight without spills) at half the resident waves
#ifndef RNT_KS_KREG_WAVES
#define RNT_KS_KREG_WAVES 4
#endif
// RNT_KS_PAIR (below, KsCfg::PAIR): off -- parity-green (the whole GPU
// suite), but the second row's 16 registers spill (k_ks_rows<u32, 8, 8>
// 92 -> 228 bytes a lane): config-4 ct-mul -1.5%, config 3 +1%, the
// 8-ciphertext rotation -4.3% (profiles/r06/ab_ks_pair.txt)
#ifndef RNT_KS_PAIR
#define RNT_KS_PAIR 0
#endif
template <class W, int LOG_C, int NP>
struct KsCfg {
  using G = RowGeo<LOG_C>;
  static constexpr int KROWS = G::RPW / NP;
  static constexpr int KPAD = ks_kpad_words<W>(G::C);
  static constexpr bool KREG = RNT_KS_KREG && sizeof(W) == 4 && G::C >= 64 && NP == 1 && G::RPW > 1;
  static constexpr bool KDOUBLE =
      !KREG && ((size_t)(G::REGION + 4 * KROWS * KPAD) * sizeof(W) <= 40u * 1024u || KROWS == 1);
  static constexpr bool KSPLIT = !KREG && sizeof(W) == 4 && G::C >= 64 && !KDOUBLE && G::P >= 2 &&
                                 (size_t)(G::REGION + 2 * KROWS * KPAD) * sizeof(W) > 40u * 1024u &&
                                 KROWS * KPAD <= G::REGION;
  static constexpr bool KEYGLDS =
      !KREG && sizeof(W) == 4 && G::C >= 64 && (NP > 1 || LOG_C >= kKsGldsWideMinLogC || KSPLIT);
  // PAIR: two source limbs a step (RNT_KS_PAIR): both rows transform
  // together (NOPS = 2, one twiddle fetch for both) and their two products
  // share one Montgomery reduction (mac2_lazy); four key-row slots (two
  // steps in flight x two limbs) beside the exchange region
  static constexpr bool PAIR = RNT_KS_PAIR && sizeof(W) == 4 && !KREG && KEYGLDS && KDOUBLE && !KSPLIT &&
                               G::P >= 2 && (size_t)(G::REGION + 8 * KROWS * KPAD) * sizeof(W) <= 40u * 1024u;
  static constexpr int KWORDS = KREG ? 0 : PAIR ? 8 * KROWS * KPAD : (KDOUBLE ? 4 : KSPLIT ? 1 : 2) * KROWS * KPAD;
  static constexpr size_t LDS_BYTES = (size_t)(G::REGION + KWORDS) * sizeof(W);
};

// 16 bytes of LDS into registers (p is 16-byte aligned by construction:
// key rows start on ks_kpad_words boundaries, and ks_pad keeps every
// thread's run of E words within a row on a 16-byte boundary).
template <class W>
__device__ __forceinline__ void ks_lds_read16(W (&o)[16 / sizeof(W)], const W* p) {
  const uint4 v = *(const uint4*)p;
  if constexpr (sizeof(W) == 4) {
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  } else {
    o[0] = (uint64_t)v.x | ((uint64_t)v.y << 32);
    o[1] = (uint64_t)v.z | ((uint64_t)v.w << 32);
  }
}

// Lazy multiply-accumulate of the u32 key-switch sum (q < 2^31): the
// accumulator lives in [0, 2q) and a term is the Montgomery product without
// its final subtraction, t = (x k + m q) / 2^32 in [0, 2q).  acc + t < 4q
// needs 33 bits: the add's carry and the borrow of subtracting 2q decide the
// select (acc + t >= 2q iff carry or no borrow), so a term costs the three
// half-rate products plus add, subtract and select, where mont_mul + add_mod
// took two more full-rate ops.  The sum is made canonical once, after the
// source-limb loop.
#ifndef RNT_KS_MAC_MEAS
#define RNT_KS_MAC_MEAS 0
#endif
__device__ __forceinline__ uint32_t mac_lazy(uint32_t acc, uint32_t x, uint32_t k, uint32_t q,
                                             uint32_t q2, uint32_t nqinv) {
  // (RNT_KS_MAC_MEAS: measurement builds only, wrong words by design -- the
  // key-switch rows with a one-op stand-in for the product, to price it)
  if constexpr (RNT_KS_MAC_MEAS) return acc + (x ^ k);
  const uint64_t T = mul64(x, k);
  const uint32_t m = (uint32_t)T * nqinv;  // -T q^-1 mod 2^32
  const uint32_t t = (uint32_t)(mad64(m, q, T) >> 32);
  uint32_t s, d;
  const bool carry = __builtin_add_overflow(acc, t, &s);
  const bool borrow = __builtin_sub_overflow(s, q2, &d);
  return (carry || !borrow) ? d : s;
}
// Two terms, one reduction: canonical x0, x1, k0, k1 < q < 2^31 give
// T = x0 k0 + x1 k1 < 2q^2 < 2^63 and T + m q < 2^64, so the shared
// Montgomery term t = (T + m q) / 2^32 < 2q^2 / 2^32 + q < 2q: the same
// [0, 2q) term mac_lazy adds, for two products (two multiply-adds, one
// reduction) instead of one.
__device__ __forceinline__ uint32_t mac2_lazy(uint32_t acc, uint32_t x0, uint32_t k0, uint32_t x1, uint32_t k1,
                                              uint32_t q, uint32_t q2, uint32_t nqinv) {
  if constexpr (RNT_KS_MAC_MEAS) return acc + (x0 ^ k0) + (x1 ^ k1);
  const uint64_t T = mad64(x1, k1, mul64(x0, k0));
  const uint32_t m = (uint32_t)T * nqinv;
  const uint32_t t = (uint32_t)(mad64(m, q, T) >> 32);
  uint32_t s, d;
  const bool carry = __builtin_add_overflow(acc, t, &s);
  const bool borrow = __builtin_sub_overflow(s, q2, &d);
  return (carry || !borrow) ? d : s;
}

// Key-switch rows.  A workgroup owns row r of target limb j for RPW
// consecutive polys p (grid: (j, r) major, poly group minor, dealt so the
// workgroups of one (j, r) share an XCD).  For every source limb i: forward
// rows of S[j][i][p], multiply-accumulate with the NTT-resident keys; then
// the inverse rows of both accumulators.  The key rows of (i, j, r) are the
// same for every poly of the workgroup, so its threads load them once per i,
// cooperatively and together with the S rows, into a double-buffered LDS
// slot, and the accumulate reads them back from LDS: one global round trip
// per source limb instead of three (S, then key_b, then key_a), and 2 key
// words per thread instead of 2E (A/B: profiles/r02_ab_ks_rows.txt).
//
// LIN (rnt_ct_linear's terms): before the inverse rows both accumulators are
// multiplied by a plaintext's NTT row -- lin.mul points at the term's plane of
// a [limb][..][N] array of Montgomery-form words (m^ 2^w mod q, limb stride
// lin.mul_ls), the same row for every poly, so the product leaves the sum's
// single factor 2^-w in place -- and with lin.accum (uniform) the inverse rows
// are added to u0/u1 instead of stored: the terms of a sum share one pair of
// accumulators and one pair of inverse column passes.  The row is read from
// global memory once per accumulator (the second read hits cache; held across
// the first inverse it would cost E more live registers).  Without LIN the
// argument is an empty struct and the kernel the one it was before it.
template <class W, bool LIN>
struct KsLinArgs {};
template <class W>
struct KsLinArgs<W, true> {
  const W* mul;
  uint64_t mul_ls;
  uint32_t accum;
};
template <class W, int LOG_C, int NP, bool LIN = false>
__global__ void __launch_bounds__(RowGeo<LOG_C>::THREADS, (KsCfg<W, LOG_C, NP>::KREG ? RNT_KS_KREG_WAVES : sizeof(W) == 4 ? RNT_KS_ROWS_WAVES : 1))
k_ks_rows(W* __restrict__ u0, W* __restrict__ u1, const W* __restrict__ S,
          const W* __restrict__ key_a, const W* __restrict__ key_b, uint64_t key_ls,
          const W* __restrict__ init0, const W* __restrict__ init1, uint64_t init_ls,
          TabPtrs<W> tp, uint32_t log_n, uint32_t L, uint32_t B, uint64_t ls, uint32_t pgroups,
          uint32_t nblocks, const W* __restrict__ d2hat, uint64_t d2hat_ls, KsLinArgs<W, LIN> lin) {
  if constexpr (LIN) d2hat = nullptr;  // no ct-mul diagonal in a linear transform's term
  using G = RowGeo<LOG_C>;
  constexpr int E = G::E;
  constexpr int C = G::C;
  // padded key row (ks_pad), rounded up to 16 bytes so every key row --
  // hence every thread's 16-byte LDS read -- starts 16-byte aligned also for
  // short rows (C = 16/32, where C + C/16 alone is 17 or 34 words)
  using K = KsCfg<W, LOG_C, NP>;
  constexpr int KPAD = K::KPAD;
  // NP polys x KROWS consecutive rows per workgroup (NP = RPW: one row r
  // for RPW polys; NP = 1: one poly, RPW rows); the key rows of a source
  // limb are staged per workgroup, KROWS of each key
  static_assert(NP >= 1 && G::RPW % NP == 0, "polys per workgroup");
  constexpr int KROWS = K::KROWS;
  constexpr bool WIDE = NP < G::RPW;
  constexpr int KPT = (2 * KROWS * C + G::THREADS - 1) / G::THREADS;  // key words per thread per i
  constexpr bool kKeyGlds = K::KEYGLDS;
  constexpr bool KDOUBLE = K::KDOUBLE;
  constexpr bool KSPLIT = K::KSPLIT;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  W* lds = (W*)smem_raw;
  // [buffers][key_b rows | key_a rows]
  W* kbuf = lds + G::REGION;
  // XCD-aware deal: hardware block b runs on XCD b % 8; consecutive logical
  // blocks (one (j, r), successive poly groups) get the same b % 8
  const uint32_t per_xcd = (nblocks + 7) / 8;
  const uint32_t wg = (blockIdx.x & 7u) * per_xcd + (blockIdx.x >> 3);
  if (wg >= nblocks) return;  // the whole workgroup: no barrier is left waiting
  const uint32_t log_r = log_n - G::LOGC;
  const uint32_t pg = wg % pgroups;
  const uint32_t jr = wg / pgroups;
  RowPos rp;
  rp.xp.slot = G::slot_of(threadIdx.x);
  rp.xp.tau = G::tau_of(threadIdx.x);
  uint32_t rbase;  // first row of the workgroup's key rows
  if constexpr (WIDE) {
    // jr = (j, row group of KROWS rows); slot = row-in-group * NP + poly-in-group
    const uint32_t lg = log_r - (uint32_t)__builtin_ctz(KROWS);
    rbase = (jr & ((1u << lg) - 1u)) * KROWS;
    rp.r = rbase + rp.xp.slot / NP;
    rp.l = jr >> lg;
    const uint32_t p = pg * NP + rp.xp.slot % NP;
    rp.active = p < B;
    rp.p = rp.active ? p : B - 1;
  } else {
    rp.r = jr & ((1u << log_r) - 1u);
    rbase = rp.r;
    rp.l = jr >> log_r;
    const uint32_t p = pg * G::RPW + rp.xp.slot;
    rp.active = p < B;
    rp.p = rp.active ? p : B - 1;  // inactive slots read a valid row, store nothing
  }
  rp.xp.heap = (1u << log_n) + rp.r * (uint32_t)G::C;
  const uint64_t N = 1ull << log_n;
  const uint32_t j = rp.l;
  const uint64_t rowoff = (uint64_t)rp.r * G::C;
  const uint64_t ibase = (uint64_t)j * init_ls + (uint64_t)rp.p * N + rowoff;
  const LimbConst<W> lc = tp.lc[j];
  const Tw<W>* tw = tp.tw + (uint64_t)j * N;
  const Tw<W>* itw = tp.itw + (uint64_t)j * N;
  const uint32_t b0 = G::base(rp.xp.tau, G::BB0);
  const uint32_t bl = G::base(rp.xp.tau, G::BBL);
  // u32: the lazy [0, 2q) accumulation (mac_lazy); u64: mont_mul + add_mod
  constexpr bool kLazy = sizeof(W) == 4;
  W nqinv = (W)0 - lc.qinv;
  asm volatile("" : "+s"(nqinv));  // keeps T * (-q^-1) one multiply (not -(T q^-1))
  const W q2 = lc.q + lc.q;
  W acc[2][E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const uint32_t pos = bl + ((uint32_t)e << G::BBL);
    acc[0][e] = init0 ? init0[ibase + pos] : (W)0;
    acc[1][e] = init1 ? init1[ibase + pos] : (W)0;
  }
  constexpr uint32_t KW = (uint32_t)(KROWS * C);  // words per key
  if constexpr (K::PAIR) {
    // the off-diagonal sources two a step (the last alone when their count
    // is odd), then the diagonal alone (the tensor's d2^ row, no transform)
    const bool dg = d2hat != nullptr && j < L;
    const uint32_t n = dg ? L - 1 : L;
    const uint32_t steps = (n + 1) / 2 + (dg ? 1u : 0u);
    auto src_of = [&](uint32_t t) { return dg && t >= j ? t + 1 : t; };
    constexpr uint32_t SEG = KW / 64;  // 64-word segments per key
    constexpr int WAVES = G::THREADS / 64;
    constexpr uint32_t SLOT = 2 * KROWS * KPAD;  // both keys' rows of one source limb
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    // both keys' rows of source limb i, global -> LDS (one segment per wave
    // instruction, as the one-limb loop below)
    auto keys_to = [&](uint32_t i, W* kb) {
      const uint64_t kbase = (uint64_t)j * key_ls + (uint64_t)i * N + (WIDE ? (uint64_t)rbase * G::C : rowoff);
#pragma unroll
      for (int m = 0; m < (int)((2 * SEG + WAVES - 1) / WAVES); ++m) {
        const uint32_t sg = wave + (uint32_t)m * WAVES;
        if (sg < 2 * SEG) {
          const uint32_t kk = sg >= SEG, rs = kk ? sg - SEG : sg;
          const W* src = (kk ? key_a : key_b) + kbase + rs * 64u + lane;
          W* dst = kb + kk * (KROWS * KPAD) + (rs / (C / 64)) * KPAD + ks_pad((rs % (C / 64)) * 64u);
          __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void*)src,
                                           (__attribute__((address_space(3))) void*)dst, 4, 0, 0);
        }
      }
    };
    auto s_row = [&](uint32_t i, W (&v)[E]) {
      const uint64_t sbase = (((uint64_t)j * L + i) * B + rp.p) * N + rowoff;
#pragma unroll
      for (int e = 0; e < E; ++e) v[e] = S[sbase + b0 + ((uint32_t)e << G::BB0)];
    };
    auto kptr = [&](const W* kb, int o) {
      return kb + o * KROWS * KPAD + (WIDE ? (rp.xp.slot / NP) * KPAD : 0u) + ks_pad(bl);
    };
#pragma unroll 1
    for (uint32_t st = 0; st < steps; ++st) {
      // key slots: two steps in flight (the transform's exchange barriers of
      // step st - 1 order every read of step st - 2's slot before this write)
      W* kb = kbuf + (st & 1u) * 2 * SLOT;
      const uint32_t t0 = 2 * st;
      if (t0 + 1 < n) {
        const uint32_t i0 = src_of(t0), i1 = src_of(t0 + 1);
        keys_to(i0, kb);
        keys_to(i1, kb + SLOT);
        // the DMA issues before the S loads, so the transform's first vmcnt
        // wait covers it and its exchange barriers publish the slot
        __builtin_amdgcn_sched_barrier(0);
        W x[2][E];
        s_row(i0, x[0]);
        s_row(i1, x[1]);
        xf_fwd<G, W, 2>(x, rp.xp, lds, tw, mod_of(lc));
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int o = 0; o < 2; ++o) {
          const W* k0 = kptr(kb, o);
          const W* k1 = kptr(kb + SLOT, o);
#pragma unroll
          for (int e0 = 0; e0 < E; e0 += 4) {
            W kv0[4], kv1[4];
            ks_lds_read16<W>(kv0, k0 + e0);
            ks_lds_read16<W>(kv1, k1 + e0);
#pragma unroll
            for (int v = 0; v < 4; ++v)
              acc[o][e0 + v] = mac2_lazy(acc[o][e0 + v], x[0][e0 + v], kv0[v], x[1][e0 + v], kv1[v], lc.q, q2, nqinv);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      } else {
        // one source: the odd one out, or the diagonal (the last step: no
        // transform, so a barrier before its key write and one after)
        const bool diag = t0 >= n;
        const uint32_t i0 = diag ? j : src_of(t0);
        if (diag) __syncthreads();
        keys_to(i0, kb);
        __builtin_amdgcn_sched_barrier(0);
        W x[1][E];
        if (diag) {
          const uint64_t hb = (uint64_t)j * d2hat_ls + (uint64_t)rp.p * N + rowoff + bl;
#pragma unroll
          for (int e = 0; e < E; ++e) x[0][e] = d2hat[hb + (uint32_t)e];
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's key DMA has landed
          __syncthreads();
        } else {
          s_row(i0, x[0]);
          xf_fwd<G, W, 1>(x, rp.xp, lds, tw, mod_of(lc));
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int o = 0; o < 2; ++o) {
          const W* kk = kptr(kb, o);
#pragma unroll
          for (int e0 = 0; e0 < E; e0 += 4) {
            W kv[4];
            ks_lds_read16<W>(kv, kk + e0);
#pragma unroll
            for (int v = 0; v < 4; ++v)
              acc[o][e0 + v] = mac_lazy(acc[o][e0 + v], x[0][e0 + v], kv[v], lc.q, q2, nqinv);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
  } else if constexpr (K::KREG) {
    // the source row of limb i: S[j][i][p] in the first pass's layout, or on
    // the diagonal the tensor's exact d2^ row in the last pass's (no
    // transform, so no LDS and no barrier that iteration: every wave passes
    // the same barriers, diag being uniform over the workgroup)
    auto src_row = [&](uint32_t i, W (&v)[E]) {
      if (d2hat != nullptr && i == j) {
        const uint64_t hb = (uint64_t)j * d2hat_ls + (uint64_t)rp.p * N + rowoff + bl;
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = d2hat[hb + (uint32_t)e];
      } else {
        const uint64_t sbase = (((uint64_t)j * L + i) * B + rp.p) * N + rowoff;
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = S[sbase + b0 + ((uint32_t)e << G::BB0)];
      }
    };
    W xn[E];
    if constexpr (RNT_KS_SPRE) src_row(0, xn);
#pragma unroll 1
    for (uint32_t i = 0; i < L; ++i) {
      W x[1][E];
      if constexpr (RNT_KS_SPRE) {
#pragma unroll
        for (int e = 0; e < E; ++e) x[0][e] = xn[e];
        if (i + 1 < L) src_row(i + 1, xn);
      } else {
        src_row(i, x[0]);
      }
      // this thread's E consecutive words (the last pass's layout, bl + e)
      // of both keys' row: 16-byte loads, consecutive across the row's threads
      W kv[2][E];
      const uint64_t kt = (uint64_t)j * key_ls + (uint64_t)i * N + rowoff + bl;
      auto load_keys = [&]() {
#pragma unroll
        for (int e = 0; e < E; e += 4) {
          const uint4 b4 = *(const uint4*)(key_b + kt + e);
          const uint4 a4 = *(const uint4*)(key_a + kt + e);
          kv[0][e] = b4.x; kv[0][e + 1] = b4.y; kv[0][e + 2] = b4.z; kv[0][e + 3] = b4.w;
          kv[1][e] = a4.x; kv[1][e + 1] = a4.y; kv[1][e + 2] = a4.z; kv[1][e + 3] = a4.w;
        }
      };
      // RNT_KS_KLATE: the key loads after the transform (32 registers fewer
      // live across it, their latency exposed)
      if constexpr (!RNT_KS_KLATE) load_keys();
      if (!(d2hat != nullptr && i == j)) xf_fwd<G, W, 1>(x, rp.xp, lds, tw, mod_of(lc));
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (RNT_KS_KLATE) load_keys();
#pragma unroll
      for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int e = 0; e < E; ++e) acc[o][e] = mac_lazy(acc[o][e], x[0][e], kv[o][e], lc.q, q2, nqinv);
      __builtin_amdgcn_sched_barrier(0);
    }
  } else {
#pragma unroll 1
  for (uint32_t i = 0; i < L; ++i) {
    // this limb's key rows (key poly i, limb j, rows rbase ..; limb stride
    // key_ls) and S rows: one batch of loads, one wait
    const uint64_t sbase = (((uint64_t)j * L + i) * B + rp.p) * N + rowoff;
    const uint64_t kbase = (uint64_t)j * key_ls + (uint64_t)i * N + (WIDE ? (uint64_t)rbase * G::C : rowoff);
    W x[1][E];
    // the diagonal (source limb i == target limb j): x is the tensor's exact
    // d2^ row, already in the last pass's layout -- no S row, no transform.
    // Without the transform's exchange barriers, one barrier before the key
    // loads (every read of the earlier limbs' key rows, and of key_a's in
    // the exchange region, is done) and one after them publish the rows
    const bool diag = d2hat != nullptr && i == j;
    if (diag) __syncthreads();
    // one key buffer: every thread's reads of the previous limb's keys
    // finish before it is rewritten
    if constexpr (!KDOUBLE) __syncthreads();
    W* kb = KDOUBLE ? kbuf + (i & 1u) * 2 * KROWS * KPAD : kbuf;
    if constexpr (kKeyGlds) {
      // u32 rows of >= 64 words: the key rows go global -> LDS directly, one
      // 64-word segment (one ks_pad run) per wave instruction, no registers
      constexpr uint32_t SEG = KW / 64;  // segments per key
      constexpr int WAVES = G::THREADS / 64;
      const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
      const uint32_t lane = threadIdx.x & 63u;
      constexpr uint32_t NK = KSPLIT ? 1 : 2;  // keys loaded here (KSPLIT: key_a after the transform)
#pragma unroll
      for (int m = 0; m < (int)((NK * SEG + WAVES - 1) / WAVES); ++m) {
        const uint32_t sg = wave + (uint32_t)m * WAVES;
        if (sg < NK * SEG) {
          const uint32_t kk = sg >= SEG, rs = kk ? sg - SEG : sg;  // key, segment within it
          const W* src = (kk ? key_a : key_b) + kbase + rs * 64u + lane;
          W* dst = kb + kk * (KROWS * KPAD) + (rs / (C / 64)) * KPAD + ks_pad((rs % (C / 64)) * 64u);
          __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void*)src,
                                           (__attribute__((address_space(3))) void*)dst, 4, 0, 0);
        }
      }
      // pin the order: the LDS-DMA key loads issue before the S loads, so the
      // (in-order) vmcnt wait for x below also covers them; the exchange
      // barriers after it then publish kb to the other waves
      __builtin_amdgcn_sched_barrier(0);
      if (diag) {
        const uint64_t hb = (uint64_t)j * d2hat_ls + (uint64_t)rp.p * N + rowoff + bl;
#pragma unroll
        for (int e = 0; e < E; ++e) x[0][e] = d2hat[hb + (uint32_t)e];
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e) x[0][e] = S[sbase + b0 + ((uint32_t)e << G::BB0)];
      }
      if constexpr (G::P < 2) {
        // no exchange barrier follows: wait for this wave's DMA explicitly
        // before the barrier below publishes kb
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    } else {
      W kr[KPT];
#pragma unroll
      for (int m = 0; m < KPT; ++m) {
        const uint32_t w = threadIdx.x + (uint32_t)m * G::THREADS;
        if (w < 2u * KW) kr[m] = w < KW ? key_b[kbase + w] : key_a[kbase + w - KW];
      }
      if (diag) {
        const uint64_t hb = (uint64_t)j * d2hat_ls + (uint64_t)rp.p * N + rowoff + bl;
#pragma unroll
        for (int e = 0; e < E; ++e) x[0][e] = d2hat[hb + (uint32_t)e];
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e) x[0][e] = S[sbase + b0 + ((uint32_t)e << G::BB0)];
      }
#pragma unroll
      for (int m = 0; m < KPT; ++m) {
        const uint32_t w = threadIdx.x + (uint32_t)m * G::THREADS;
        if (w < 2u * KW) {
          const uint32_t wk = w < KW ? w : w - KW;  // word within its key's rows
          kb[(w < KW ? 0u : KROWS * KPAD) + (wk / C) * KPAD + ks_pad(wk & (C - 1))] = kr[m];
        }
      }
    }
    // the transform's LDS exchange ends in barriers that publish kb (and
    // order the reads of this slot two limbs ago before this write); a
    // single-pass row has none, so it gets one here
    if (diag) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's key DMA has landed
      __syncthreads();
    } else {
      if constexpr (G::P < 2) __syncthreads();
      xf_fwd<G, W, 1>(x, rp.xp, lds, tw, mod_of(lc));
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (KSPLIT) {
      // the transform's last exchange has ended in a barrier: the exchange
      // region takes key_a's rows while acc0 takes key_b's
      constexpr uint32_t SEG = KW / 64;
      constexpr int WAVES = G::THREADS / 64;
      const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
      const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
      for (int m = 0; m < (int)((SEG + WAVES - 1) / WAVES); ++m) {
        const uint32_t rs = wave + (uint32_t)m * WAVES;
        if (rs < SEG) {
          const W* src = key_a + kbase + rs * 64u + lane;
          W* dst = lds + (rs / (C / 64)) * KPAD + ks_pad((rs % (C / 64)) * 64u);
          __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void*)src,
                                           (__attribute__((address_space(3))) void*)dst, 4, 0, 0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // the last pass leaves a thread's E values at consecutive positions
    // (G::BBL == 0): the keys come back 16 bytes at a time, one key after
    // the other
    static_assert(G::BBL == 0, "last row pass distribution");
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      if (KSPLIT && o == 1) {
        // every wave's key_a rows have landed and are visible
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
      }
      const W* kk = (KSPLIT && o == 1 ? lds : kb + o * KROWS * KPAD) + (WIDE ? (rp.xp.slot / NP) * KPAD : 0u) +
                    ks_pad(bl);
      constexpr int V = 16 / sizeof(W);
#pragma unroll
      for (int e0 = 0; e0 < E; e0 += V) {
        W kv[V];
        if constexpr (E % V == 0) {
          ks_lds_read16<W>(kv, kk + e0);
        } else {
#pragma unroll
          for (int v = 0; v < V; ++v) kv[v] = e0 + v < E ? kk[e0 + v] : (W)0;
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
          if (e0 + v >= E) continue;
          if constexpr (kLazy)
            acc[o][e0 + v] = mac_lazy(acc[o][e0 + v], x[0][e0 + v], kv[v], lc.q, q2, nqinv);
          else
            acc[o][e0 + v] = add_mod<W>(acc[o][e0 + v], mont_mul<W>(x[0][e0 + v], kv[v], lc.q, lc.qinv), lc.q);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  }
  // (KSPLIT: every thread's reads of the last key_a rows end before the
  // inverse's exchanges write that region)
  if constexpr (KSPLIT) __syncthreads();
  // the two accumulators' inverse rows one after the other (half the live
  // registers of a two-operand pass).  The thread coordinates pass through
  // an opaque copy, so the inverse passes' twiddle and store addresses are
  // derived here rather than computed before the loop and spilled across it
  XPos xq = rp.xp;
  uint32_t pq = rp.p;
  asm volatile("" : "+v"(xq.tau), "+v"(pq));
  const uint64_t oq = (uint64_t)j * ls + (uint64_t)pq * N + rowoff;
  const uint32_t b0q = G::base(xq.tau, G::BB0);
  // (LIN lives inside this loop as discarded statements: written as a block
  // of its own in front of it, the code of the existing instantiations -- and
  // of k_row and k_tensor_rows -- moved.  The u64 LIN rows of 128 words and
  // more outgrow the compiler's full-unroll limit here and keep their two
  // accumulators in scratch, 272 bytes a lane written once and read once.)
#pragma unroll
  for (int o = 0; o < 2; ++o) {
    W v[1][E];
#pragma unroll
    for (int e = 0; e < E; ++e) v[0][e] = kLazy ? csub<W>(acc[o][e], lc.q) : acc[o][e];
    if constexpr (LIN) {
      // the plaintext's row at this thread's accumulator positions (the seed
      // loads' pattern; no poly index: one row serves the batch)
      const W* mr = lin.mul + (uint64_t)j * lin.mul_ls + rowoff;
#pragma unroll
      for (int e = 0; e < E; ++e)
        v[0][e] = mont_mul<W>(v[0][e], mr[bl + ((uint32_t)e << G::BBL)], lc.q, lc.qinv);
    }
    xf_inv<G, W, 1>(v, xq, lds, itw, mod_of(lc));
    W* uo = o == 0 ? u0 : u1;
    if constexpr (LIN) {
      // a later term of the sum: add the rows already there (accum is
      // uniform; the loads are issued together, ahead of the adds)
      if (rp.active && lin.accum) {
        W old[E];
#pragma unroll
        for (int e = 0; e < E; ++e) old[e] = uo[oq + b0q + ((uint32_t)e << G::BB0)];
#pragma unroll
        for (int e = 0; e < E; ++e) v[0][e] = add_mod<W>(old[e], v[0][e], lc.q);
      }
    }
    if (rp.active) {
#pragma unroll
      for (int e = 0; e < E; ++e) uo[oq + b0q + ((uint32_t)e << G::BB0)] = v[0][e];
    }
  }
}

// Whole-plane key-switch (2^10 <= N <= 2^13): a workgroup owns target
// limb j of RPW polys, each plane one row (RowGeo<log N>, as k_row's WHOLE
// form).  For every source limb i it reduces the coefficient-domain plane
// d_i mod q_j, runs the whole forward transform and multiply-accumulates
// with the NTT-resident keys (each thread's 16 consecutive words of both,
// straight from memory: at one poly per row no key row is shared), then
// runs the whole inverse of both accumulators with the folded n^-1 2^w of
// the Montgomery sums and stores the coefficient-domain result (+ the
// addend on the first).  No S intermediate and no column launches: per poly
// and target limb the source planes and the key planes in, two planes out,
// in one launch (the four-step path writes and reads S, L planes per target
// limb, and runs three more launches).
template <class W, int LOG_N>
__global__ void __launch_bounds__(RowGeo<LOG_N>::THREADS, sizeof(W) == 4 ? kKsMinWaves : 1)
k_ks_whole(W* __restrict__ out0, W* __restrict__ out1, uint64_t out_ls, const W* __restrict__ src,
           uint64_t src_ls, const W* __restrict__ key_a, const W* __restrict__ key_b, uint64_t key_ls,
           const W* __restrict__ init0, const W* __restrict__ init1, uint64_t init_ls,
           const W* __restrict__ add0, TabPtrs<W> tp, uint32_t L, uint32_t B) {
  using G = RowGeo<LOG_N>;
  constexpr int E = G::E;
  static_assert(G::BBL == 0 && E == 16, "last pass: 16 consecutive words a thread");
  constexpr uint64_t N = 1ull << LOG_N;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  W* lds = (W*)smem_raw;
  XPos xp;
  xp.slot = G::slot_of(threadIdx.x);
  xp.tau = G::tau_of(threadIdx.x);
  xp.heap = 1u << LOG_N;
  const uint32_t j = blockIdx.y;
  const uint32_t pp = blockIdx.x * G::RPW + xp.slot;
  const bool active = pp < B;
  const uint32_t p = active ? pp : B - 1;  // inactive slots read a valid plane, store nothing
  const LimbConst<W> lc = tp.lc[j];
  const Tw<W>* tw = tp.tw + (uint64_t)j * N;
  const Tw<W>* itw = tp.itw + (uint64_t)j * N;
  const uint32_t b0 = G::base(xp.tau, G::BB0);
  const uint32_t bl = G::base(xp.tau, G::BBL);
  constexpr bool kLazy = sizeof(W) == 4;
  W nqinv = (W)0 - lc.qinv;
  asm volatile("" : "+s"(nqinv));
  const W q2 = lc.q + lc.q;
  W acc[2][E];
  const uint64_t ibase = (uint64_t)j * init_ls + (uint64_t)p * N + bl;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    acc[0][e] = init0 ? init0[ibase + e] : (W)0;
    acc[1][e] = init1 ? init1[ibase + e] : (W)0;
  }
  auto ld16 = [](W (&o)[E], const W* q) {
    constexpr int V = 16 / (int)sizeof(W);
#pragma unroll
    for (int e0 = 0; e0 < E; e0 += V) {
      const uint4 v = *(const uint4*)(q + e0);
      if constexpr (sizeof(W) == 4) {
        o[e0] = v.x; o[e0 + 1] = v.y; o[e0 + 2] = v.z; o[e0 + 3] = v.w;
      } else {
        o[e0] = (uint64_t)v.x | ((uint64_t)v.y << 32);
        o[e0 + 1] = (uint64_t)v.z | ((uint64_t)v.w << 32);
      }
    }
  };
  auto mac = [&](W (&a)[E], const W (&x)[E], const W (&k)[E]) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if constexpr (kLazy)
        a[e] = mac_lazy(a[e], x[e], k[e], lc.q, q2, nqinv);
      else
        a[e] = add_mod<W>(a[e], mont_mul<W>(x[e], k[e], lc.q, lc.qinv), lc.q);
    }
  };
#pragma unroll 1
  for (uint32_t i = 0; i < L; ++i) {
    const W* kb = key_b + (uint64_t)j * key_ls + (uint64_t)i * N + bl;
    const W* ka = key_a + (uint64_t)j * key_ls + (uint64_t)i * N + bl;
    W x[1][E];
    const W* sp = src + (uint64_t)i * src_ls + (uint64_t)p * N + b0;
#pragma unroll
    for (int e = 0; e < E; ++e) x[0][e] = shoup_mul<W>(sp[(uint32_t)e << G::BB0], (W)1, lc.one_p, lc.q);  // d_i mod q_j
    xf_fwd<G, W, 1>(x, xp, lds, tw, mod_of(lc));
    W kv[E];
    ld16(kv, kb);
    mac(acc[0], x[0], kv);
    ld16(kv, ka);
    mac(acc[1], x[0], kv);
  }
  // the thread coordinates pass through an opaque copy, so the inverse's
  // addresses are derived here rather than held (spilled) across the loop
  XPos xq = xp;
  uint32_t pq = p;
  asm volatile("" : "+v"(xq.tau), "+v"(pq));
  const uint64_t obase = (uint64_t)j * out_ls + (uint64_t)pq * N + G::base(xq.tau, G::BB0);
  // the two accumulators' inverses one after the other (written out twice:
  // a loop over them is not unrolled, and acc would be indexed at run time)
  auto finish = [&](W (&a)[E], W* dst, const W* add) {
    W v[1][E];
#pragma unroll
    for (int e = 0; e < E; ++e) v[0][e] = kLazy ? csub<W>(a[e], lc.q) : a[e];
    xf_inv<G, W, 1, true>(v, xq, lds, itw, mod_of(lc), Fold<W>{lc.c1r, lc.c1r_p, lc.c2r, lc.c2r_p});
    if (active) {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const uint64_t pos = obase + ((uint32_t)e << G::BB0);
        dst[pos] = add ? add_mod<W>(v[0][e], add[pos], lc.q) : v[0][e];
      }
    }
  };
  finish(acc[0], out0, add0);
  finish(acc[1], out1, nullptr);
}

template <class W, int LOG_C, int NP>
static hipError_t ks_rows_launch(const Launch& k, void* u0, void* u1, uint64_t ls, const void* S,
                                 const void* key_a, const void* key_b, uint64_t key_ls,
                                 const void* init0, const void* init1, uint64_t init_ls,
                                 const KsLin* lin) {
  using G = RowGeo<LOG_C>;
  constexpr int KROWS = G::RPW / NP;
  constexpr size_t KPADB = (size_t)ks_kpad_words<W>(G::C) * sizeof(W);
  const Geom g = geom_for(k.t->log_n);
  if (k.L == 0 || k.B == 0) return hipSuccess;
  if (g.r % KROWS) return hipErrorInvalidValue;
  // KREG's 16-byte key loads: key planes on 16-byte boundaries
  if (KsCfg<W, LOG_C, NP>::KREG && ((((uintptr_t)key_a | (uintptr_t)key_b) & 15u) || (key_ls & 3u)))
    return hipErrorInvalidValue;
  // one workgroup per (target limb, group of KROWS rows, group of NP polys)
  const uint64_t pgroups = (k.B + NP - 1) / NP;
  const uint64_t blocks = (uint64_t)k.L * (g.r / KROWS) * pgroups;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  const unsigned launched = (unsigned)((blocks + 7) / 8 * 8);  // whole XCD rounds
  // exchange region + one or two buffers of {key_b, key_a} x KROWS rows
  // (the kernel's KDOUBLE rule)
  const size_t lds = KsCfg<W, LOG_C, NP>::LDS_BYTES;
  static_assert(KsCfg<W, LOG_C, NP>::KPAD * sizeof(W) == KPADB, "key row pad");
  if (lin != nullptr) {
    // rnt_ct_linear's term: the same grid, the plaintext row and the
    // accumulate flag in place of the ct-mul diagonal
    if (k.d2hat != nullptr || lin->mul == nullptr) return hipErrorInvalidValue;
    hipError_t e = allow_lds(k_ks_rows<W, LOG_C, NP, true>, lds);
    if (e != hipSuccess) return e;
    const KsLinArgs<W, true> la{(const W*)lin->mul, lin->mul_ls, lin->accum};
    hipLaunchKernelGGL((k_ks_rows<W, LOG_C, NP, true>), dim3(launched), dim3(G::THREADS), lds, k.s,
                       (W*)u0, (W*)u1, (const W*)S, (const W*)key_a, (const W*)key_b, key_ls,
                       (const W*)init0, (const W*)init1, init_ls, tab_ptrs<W>(k.t), g.log_n,
                       (uint32_t)k.src_limbs(), (uint32_t)k.B, ls, (uint32_t)pgroups,
                       (uint32_t)blocks, (const W*)nullptr, (uint64_t)0, la);
    return hipGetLastError();
  }
  hipError_t e = allow_lds(k_ks_rows<W, LOG_C, NP>, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_ks_rows<W, LOG_C, NP>), dim3(launched), dim3(G::THREADS), lds, k.s,
                     (W*)u0, (W*)u1, (const W*)S, (const W*)key_a, (const W*)key_b, key_ls,
                     (const W*)init0, (const W*)init1, init_ls, tab_ptrs<W>(k.t), g.log_n,
                     (uint32_t)k.src_limbs(), (uint32_t)k.B, ls, (uint32_t)pgroups,
                     (uint32_t)blocks, (const W*)k.d2hat, k.d2hat_ls, KsLinArgs<W, false>{});
  return hipGetLastError();
}

// Polys per workgroup: the poly-per-slot grid (NP = RPW) shares each key
// row among RPW polys but leaves slots idle when RPW does not divide B.
// u32 rows of >= 64 words pick, among NP = RPW and smaller powers of two
// (2..8 for the configs' 2^8- and 2^9-word rows, 1 for every row length),
// the one that fills the most row slots, the larger on a tie (more key
// sharing).  B < RPW/2 used to run at B/RPW of the grid.
template <class W, int LOG_C>
static hipError_t ks_rows_pick(const Launch& k, void* u0, void* u1, uint64_t ls, const void* S,
                               const void* key_a, const void* key_b, uint64_t key_ls,
                               const void* init0, const void* init1, uint64_t init_ls,
                               const KsLin* lin) {
  using G = RowGeo<LOG_C>;
  constexpr int RPW = G::RPW;
  const Geom g = geom_for(k.t->log_n);
  // NP = polys per workgroup (each key row is loaded once for NP polys).
  // Take the largest NP whose grid fills at least 90% of its row slots:
  // slot fill alone would pick NP = 1 (always 100% full, no key sharing,
  // the most expensive grid) for every odd batch, e.g. a 63-poly last chunk
  // of a 1023-ciphertext batch.  Below that fill (small batches, B < RPW
  // mostly) the best-filled grid wins, the larger NP on a tie.
  int np = RPW;
  if (sizeof(W) == 4 && G::C >= 64 && RPW > 1) {
    double best = -1.0;
    int best_np = RPW;
    bool chosen = false;
    for (int c = RPW; c >= 1; c >>= 1) {
      const bool have = c == RPW || c == 1 || ((LOG_C == 8 || LOG_C == 9) && c <= 8);
      if (!have || g.r % (RPW / c)) continue;
      const double fill = (double)k.B / (double)(((k.B + c - 1) / c) * c);
      if (fill >= 0.9) {
        np = c;
        chosen = true;
        break;
      }
      if (fill > best + 1e-9) { best = fill; best_np = c; }
    }
    if (!chosen) np = best_np;
  }
#define RNT_NP(V) \
  if (np == (V) && RPW % (V) == 0) \
    return ks_rows_launch<W, LOG_C, (RPW % (V) == 0 ? (V) : RPW)>(k, u0, u1, ls, S, key_a, key_b, key_ls, init0, init1, init_ls, lin);
  if constexpr (sizeof(W) == 4 && G::C >= 64 && RPW > 1) {
    RNT_NP(1)
    if constexpr (LOG_C == 8 || LOG_C == 9) {
      RNT_NP(2)
      RNT_NP(4)
      RNT_NP(8)
    }
  }
#undef RNT_NP
  return ks_rows_launch<W, LOG_C, RPW>(k, u0, u1, ls, S, key_a, key_b, key_ls, init0, init1, init_ls, lin);
}

template <class W>
static hipError_t ks_rows_t(const Launch& k, void* u0, void* u1, uint64_t ls, const void* S,
                            const void* key_a, const void* key_b, uint64_t key_ls,
                            const void* init0, const void* init1, uint64_t init_ls,
                            const KsLin* lin) {
  const Geom g = geom_for(k.t->log_n);
#define RNT_L(C) \
  return ks_rows_pick<W, C>(k, u0, u1, ls, S, key_a, key_b, key_ls, init0, init1, init_ls, lin)
  RNT_DISPATCH_LOGC(g.log_c, RNT_L)
#undef RNT_L
  return hipErrorInvalidValue;
}

hipError_t launch_ks_rows(const Launch& k, void* u0, void* u1, uint64_t u_ls, const void* S,
                          const void* key_a, const void* key_b, uint64_t key_ls,
                          const void* init0, const void* init1, uint64_t init_ls) {
  return by_word(k, [&](auto w) {
    return ks_rows_t<decltype(w)>(k, u0, u1, u_ls, S, key_a, key_b, key_ls, init0, init1, init_ls, nullptr);
  });
}
hipError_t launch_ks_rows_lin(const Launch& k, void* u0, void* u1, uint64_t u_ls, const void* S,
                              const void* key_a, const void* key_b, uint64_t key_ls,
                              const void* init0, const void* init1, uint64_t init_ls, const KsLin& lin) {
  return by_word(k, [&](auto w) {
    return ks_rows_t<decltype(w)>(k, u0, u1, u_ls, S, key_a, key_b, key_ls, init0, init1, init_ls, &lin);
  });
}

template <class W>
static hipError_t ks_whole_t(const Launch& k, void* out0, void* out1, uint64_t out_ls, const void* src,
                             uint64_t src_ls, const void* key_a, const void* key_b, uint64_t key_ls,
                             const void* init0, const void* init1, uint64_t init_ls, const void* add0) {
  if (k.L == 0 || k.B == 0) return hipSuccess;
  if (k.L > 65535) return hipErrorInvalidConfiguration;
#define RNT_W(C)                                                                                        \
  case C: {                                                                                             \
    using G = RowGeo<C>;                                                                                \
    const size_t lds = row_lds<W, C>(1);                                                                \
    hipError_t e = allow_lds(k_ks_whole<W, C>, lds);                                                    \
    if (e != hipSuccess) return e;                                                                      \
    const dim3 grid((unsigned)((k.B + G::RPW - 1) / G::RPW), (unsigned)k.L);                           \
    hipLaunchKernelGGL((k_ks_whole<W, C>), grid, dim3(G::THREADS), lds, k.s, (W*)out0, (W*)out1, out_ls,   \
                       (const W*)src, src_ls, (const W*)key_a, (const W*)key_b, key_ls, (const W*)init0,  \
                       (const W*)init1, init_ls, (const W*)add0, tab_ptrs<W>(k.t), (uint32_t)k.src_limbs(), \
                       (uint32_t)k.B);                                                                  \
    return hipGetLastError();                                                                           \
  }
  switch (k.t->log_n) {
    RNT_W(10)
    RNT_W(11)
    RNT_W(12)
    RNT_W(13)
    default: return hipErrorInvalidValue;  // ks_whole_ok
  }
#undef RNT_W
}

bool ks_whole_ok(const Tables* t) {
  return t->plane != 0 && !t->wide && t->log_n >= 10 && t->log_n <= kKsWholeMaxLogN;
}
hipError_t launch_ks_whole(const Launch& k, void* out0, void* out1, uint64_t out_ls, const void* src,
                           uint64_t src_ls, const void* key_a, const void* key_b, uint64_t key_ls,
                           const void* init0, const void* init1, uint64_t init_ls, const void* add0) {
  if (k.t->wide) return hipErrorInvalidValue;  // ks_whole_ok
  return ks_whole_t<uint32_t>(k, out0, out1, out_ls, src, src_ls, key_a, key_b, key_ls, init0, init1, init_ls, add0);
}

// ---------------------------------------------------------------------------
// the ciphertext tensor product (engine.rs:480-493): k_tensor_rows
// ---------------------------------------------------------------------------

// 4 waves per SIMD (<= 128 VGPRs; unconstrained it takes 134-154 and runs
// at 3): tensor_rows 1.74 -> 1.64 ms per 64 cts (profiles/r02_ab_tensor_waves.txt)
constexpr int kTensorMinWaves = 4;
// WHOLE (2^10 <= N = 2^LOG_C <= 2^13): a row is the whole plane, as in k_row's
// WHOLE form, so the four operands come in coefficient domain, d0^ and d1^
// go out NTT-resident and d2 in coefficient domain (its inverse's top stage
// applies the folded n^-1 2^32 of the Montgomery product): the tensor step
// of a ct-mul is this one launch, 4 planes in and 3 out, without the two
// column launches before it and d2's column inverse after it.
template <class W, int LOG_C, bool WHOLE = false>
__global__ void __launch_bounds__(RowGeo<LOG_C>::THREADS, sizeof(W) == 4 ? kTensorMinWaves : 1)
k_tensor_rows(W* __restrict__ d0hat, W* __restrict__ d1hat, W* __restrict__ d2row,
              const W* __restrict__ c0, const W* __restrict__ c1, const W* __restrict__ c0p,
              const W* __restrict__ c1p, TabPtrs<W> tp, uint32_t log_n, uint32_t B, uint64_t ls,
              uint64_t rows_total, uint64_t in_ls, W* __restrict__ d2hat) {
  using G = RowGeo<LOG_C>;
  constexpr int E = G::E;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  W* lds = (W*)smem_raw;
  const RowPos rp = row_pos_pfast<G>(log_n, B, rows_total);  // shared twiddles, as in k_row
  const uint64_t N = 1ull << log_n;
  const uint64_t pr = (uint64_t)rp.p * N + (uint64_t)rp.r * G::C;
  const uint64_t base = (uint64_t)rp.l * ls + pr;      // outputs
  const uint64_t ibase = (uint64_t)rp.l * in_ls + pr;  // operands
  const LimbConst<W> lc = tp.lc[rp.l];
  const Tw<W>* tw = tp.tw + (uint64_t)rp.l * N;
  const Tw<W>* itw = tp.itw + (uint64_t)rp.l * N;
  const uint32_t b0 = G::base(rp.xp.tau, G::BB0);
  const uint32_t bl = G::base(rp.xp.tau, G::BBL);
  W a[2][E], b[2][E];
#pragma unroll
  for (int i = 0; i < E; ++i) {
    const uint32_t e = b0 + ((uint32_t)i << G::BB0);
    a[0][i] = c0[ibase + e];
    a[1][i] = c1[ibase + e];
  }
  xf_fwd<G, W, 2>(a, rp.xp, lds, tw, mod_of(lc));
#pragma unroll
  for (int i = 0; i < E; ++i) {
    const uint32_t e = b0 + ((uint32_t)i << G::BB0);
    b[0][i] = c0p[ibase + e];
    b[1][i] = c1p[ibase + e];
  }
  xf_fwd<G, W, 2>(b, rp.xp, lds, tw, mod_of(lc));
  W d2[1][E];
  W o0[E], o1[E];
  W nqi = (W)0 - lc.qinv;
  asm volatile("" : "+v"(nqi));  // one multiply per REDC (see mont_mul_nq)
#pragma unroll
  for (int i = 0; i < E; ++i) {
    const W q = lc.q, qi = lc.qinv;
    W d0, d1;
    if constexpr (sizeof(W) == 4) {
      d0 = mont_mul_nq(a[0][i], b[0][i], q, nqi);
      // one REDC of the two-product sum: T < 2q^2 and T + m q < 2^64, the
      // result (T + m q) / 2^32 < 2q (q < 2^31)
      const uint64_t T = mad64(a[1][i], b[0][i], mul64(a[0][i], b[1][i]));
      const uint32_t m = (uint32_t)T * nqi;
      d1 = csub<uint32_t>((uint32_t)(mad64(m, q, T) >> 32), q);
      d2[0][i] = mont_mul_nq(a[1][i], b[1][i], q, nqi);
    } else {
      d0 = mont_mul<W>(a[0][i], b[0][i], q, qi);
      d1 = add_mod<W>(mont_mul<W>(a[0][i], b[1][i], q, qi), mont_mul<W>(a[1][i], b[0][i], q, qi), q);
      d2[0][i] = mont_mul<W>(a[1][i], b[1][i], q, qi);
    }
    o0[i] = d0;
    o1[i] = d1;
  }
  // the last pass leaves a thread's E words consecutive (G::BBL == 0): the
  // outputs go as 16-byte stores (four 4-byte stores 64 bytes apart per lane
  // before: the exact d2^ as a third such stream cost the config-3 tensor
  // 44%, profiles/r06/ab_ks_diag.txt)
  static_assert(G::BBL == 0, "consecutive output words");
  if (rp.active && (E * sizeof(W)) % 16 != 0) {  // rows shorter than 16 bytes a thread
#pragma unroll
    for (int i = 0; i < E; ++i) {
      d0hat[base + bl + i] = o0[i];
      d1hat[base + bl + i] = o1[i];
      if (d2hat != nullptr) d2hat[base + bl + i] = shoup_mul<W>(d2[0][i], lc.rmod, lc.rmod_p, lc.q);
    }
  } else if (rp.active) {
    constexpr int V = 16 / sizeof(W) < E ? 16 / sizeof(W) : E;
    uint4* p0 = (uint4*)(d0hat + base + bl);
    uint4* p1 = (uint4*)(d1hat + base + bl);
#pragma unroll
    for (int t = 0; t < E / V; ++t) {
      p0[t] = *(const uint4*)&o0[t * V];
      p1[t] = *(const uint4*)&o1[t * V];
    }
    if (d2hat != nullptr) {
      // the exact d2^ (times 2^w by a Shoup product): the key-switch's own
      // source-limb-i transform of target limb i (its diagonal, k_ks_rows)
      W h[E];
#pragma unroll
      for (int i = 0; i < E; ++i) h[i] = shoup_mul<W>(d2[0][i], lc.rmod, lc.rmod_p, lc.q);
      uint4* ph = (uint4*)(d2hat + base + bl);
#pragma unroll
      for (int t = 0; t < E / V; ++t) ph[t] = *(const uint4*)&h[t * V];
    }
  }
  xf_inv<G, W, 1, WHOLE>(d2, rp.xp, lds, itw, mod_of(lc),
                         WHOLE ? Fold<W>{lc.c1r, lc.c1r_p, lc.c2r, lc.c2r_p} : Fold<W>{});
  if (rp.active) {
#pragma unroll
    for (int i = 0; i < E; ++i) d2row[base + b0 + ((uint32_t)i << G::BB0)] = d2[0][i];
  }
}

template <class W, int LOG_C, bool WHOLE = false>
static hipError_t tensor_rows_launch(const Launch& k, void* d0hat, void* d1hat, void* d2row,
                                     const void* c0, const void* c1, const void* c0p,
                                     const void* c1p, uint64_t ls, uint64_t in_ls) {
  using G = RowGeo<LOG_C>;
  const Geom g = geom_for(k.t->log_n);
  const uint64_t rows = (uint64_t)k.L * k.B * (WHOLE ? 1 : g.r);
  if (rows == 0) return hipSuccess;
  const unsigned blocks = (unsigned)((rows + G::RPW - 1) / G::RPW);
  const size_t lds = row_lds<W, LOG_C>(2);
  hipError_t e = allow_lds(k_tensor_rows<W, LOG_C, WHOLE>, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_tensor_rows<W, LOG_C, WHOLE>), dim3(blocks), dim3(G::THREADS), lds, k.s,
                     (W*)d0hat, (W*)d1hat, (W*)d2row, (const W*)c0, (const W*)c1,
                     (const W*)c0p, (const W*)c1p, tab_ptrs<W>(k.t),
                     WHOLE ? (uint32_t)LOG_C : g.log_n, (uint32_t)k.B, ls, rows, in_ls,
                     (W*)(WHOLE ? nullptr : k.d2hat));  // (its stride is the outputs' ls)
  return hipGetLastError();
}

template <class W>
static hipError_t tensor_rows_t(const Launch& k, void* d0hat, void* d1hat, void* d2row,
                                const void* c0, const void* c1, const void* c0p,
                                const void* c1p, uint64_t ls) {
  const Geom g = geom_for(k.t->log_n);
#define RNT_L(C) return tensor_rows_launch<W, C>(k, d0hat, d1hat, d2row, c0, c1, c0p, c1p, ls, ls)
  RNT_DISPATCH_LOGC(g.log_c, RNT_L)
#undef RNT_L
  return hipErrorInvalidValue;
}

template <class W>
static hipError_t tensor_whole_t(const Launch& k, void* d0hat, void* d1hat, void* d2, uint64_t ls,
                                 const void* c0, const void* c1, const void* c0p, const void* c1p,
                                 uint64_t in_ls) {
#define RNT_W(C)                                                                                     \
  case C:                                                                                            \
    if constexpr (sizeof(W) == 8 && C > 12) return hipErrorInvalidValue; /* tensor_whole_ok */      \
    else return tensor_rows_launch<W, C, true>(k, d0hat, d1hat, d2, c0, c1, c0p, c1p, ls, in_ls);
  switch (k.t->log_n) {
    RNT_W(10)
    RNT_W(11)
    RNT_W(12)
    RNT_W(13)
  }
#undef RNT_W
  return hipErrorInvalidValue;  // tensor_whole_ok
}
// (the u64 tensor holds four operand planes: N <= 2^12 only)
bool tensor_whole_ok(const Tables* t) {
  return whole_ok(t, 2) && t->log_n <= kKsWholeMaxLogN && !(t->wide && t->log_n > 12);
}
hipError_t launch_tensor_whole(const Launch& k, void* d0hat, void* d1hat, void* d2, uint64_t ls,
                               const void* c0, const void* c1, const void* c0p, const void* c1p,
                               uint64_t in_ls) {
  return by_word(k, [&](auto w) { return tensor_whole_t<decltype(w)>(k, d0hat, d1hat, d2, ls, c0, c1, c0p, c1p, in_ls); });
}
hipError_t launch_tensor_rows(const Launch& k, void* d0hat, void* d1hat, void* d2row,
                              const void* c0, const void* c1, const void* c0p, const void* c1p,
                              uint64_t ls) {
  return by_word(k, [&](auto w) { return tensor_rows_t<decltype(w)>(k, d0hat, d1hat, d2row, c0, c1, c0p, c1p, ls); });
}

}  // namespace rnt
