// rnt_internal.hpp -- private types shared by the C-ABI layer (rnt_api.cpp)
// and the kernel units (rnt_col / rnt_rows / rnt_kernels /
// rnt_raise / rnt_plane / rnt_mfma .hip).
//
// Device layout (private):
//   A buffer of B polynomials over L limbs is one allocation of W words laid
//   out [L][B][N] (limb-major, so a limb shard is contiguous and one prime's
//   twiddles serve a whole contiguous launch range).  W = uint32_t when every
//   modulus is < 2^31, else uint64_t.
//   NTT-domain data is stored in bit-reversed order of the natural
//   evaluation index (the output order of the merged negacyclic CT
//   transform), i.e. device[brv(k)] = a(psi^(2k+1)).  Upload / download
//   permute to and from the reference's natural order.
//
// Transform decomposition: N = R * C.  The column pass does the top log2(R)
// CT stages (a stride-C radix-R butterfly network per column, in
// registers); the row pass does the remaining log2(C) stages per row of C
// contiguous words through LDS in radix-16 register passes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace rnt {

constexpr int kMaxLogN = 17;
constexpr int kRowElems = 16;  // elements per thread per operand in the row pass
// threads per row-pass workgroup (at least one row's C/16 threads)
constexpr int kRowThreads = 256;

template <class W>
struct LimbConst {
  W q;       // modulus
  W qinv;    // q^-1 mod 2^w (Montgomery)
  W one_p;   // floor(2^w / q): Shoup companion of 1 (canonical reduction of x < 2^w)
  W rmod;    // 2^w mod q
  W rmod_p;
  W c1;      // n^-1                      (last inverse stage, plain)
  W c1_p;
  W c2;      // psi_inv_rev[1] * n^-1
  W c2_p;
  W c1r;     // n^-1 * 2^w                (last inverse stage, Montgomery-folded)
  W c1r_p;
  W c2r;     // psi_inv_rev[1] * n^-1 * 2^w
  W c2r_p;
  W c1t;     // 4 n^-1 * 2^w             (last stage after a product truncated two stages early)
  W c1t_p;
  W c2t;     // psi_inv_rev[1] * 4 n^-1 * 2^w
  W c2t_p;
};

// A twiddle and its Shoup companion, interleaved so one load fetches both.
template <class W>
struct alignas(2 * sizeof(W)) Tw {
  W w;  // psi^{+-brv(g)} mod q
  W p;  // floor(w * 2^w / q)
};

// Shared, immutable device tables of a root basis.  drop_last views hold a
// shared_ptr to the same tables (no copy, unlike basis.rs:130-133).
// Device pointers of the centred-CRT constants (rnt_kernels.hip k_crt).
struct CrtConsts {
  const uint32_t* qi_words;  // [L][MW]  Q / q_l
  const uint32_t* q_words;   // [MW]     Q
  const uint32_t* qh_words;  // [MW]     floor(Q / 2)
  const uint64_t* inv;       // [L]      (Q/q_l)^-1 mod q_l
  const uint64_t* inv_p;     // [L]      its Shoup companion (device word width)
  const double* rq;          // [L]      1 / q_l
};
struct CrtDev {
  void* dev = nullptr;
  uint32_t mw = 0;
  CrtConsts cc{};
};

// Device pointers of the hybrid key-switch constants (k_modup, k_moddown;
// words of the basis' width).  Lv ciphertext limbs q_j, K special limbs p_k
// (the key basis' limbs Lv .. Lv + K - 1), beta digits of alpha limbs.
struct HybridConsts {
  const void* yinv = nullptr;   // [Lv]  (Q_d / q_i)^-1 mod q_i, d the digit of i
  const void* yinvp = nullptr;  //       Shoup companions (of every table below too)
  const void* conv = nullptr;   // [beta][alpha][Lv + K]  (Q_d / q_i) 2^w mod m_t
  const void* convp = nullptr;
  const void* pinv = nullptr;   // [K]  (P / p_k)^-1 mod p_k
  const void* pinvp = nullptr;
  const void* pq = nullptr;     // [K][Lv]  (P / p_k) mod q_j
  const void* pqp = nullptr;
  const void* Pinv = nullptr;   // [Lv]  P^-1 mod q_j
  const void* Pinvp = nullptr;
  const void* Pw = nullptr;     // [Lv]  P 2^w mod q_j (k_hoist_mac_seed)
  const void* Pwp = nullptr;
  uint32_t Lv = 0, K = 0, alpha = 0, beta = 0;
};
struct HybridDev {
  size_t LE = 0, Lv = 0, alpha = 0;
  size_t level = 0, gap = 0;  // the key context's limb map (a level view; else UINT32_MAX, 0)
  void* dev = nullptr;
  HybridConsts hc{};
};

// The constants of rnt_mod_raise (rnt_raise.hip k_mod_raise) from the first
// l0 <= kRaiseMax limbs of a basis onto all of it.  RaiseDigits goes to the
// kernel by value (words of the basis' width held in u64): for i >= 1 the
// Garner digit is d_i = (x_i - sum_{k<i} d_k pre[i][k]) ginv[i] mod q_i with
// pre[i][k] = q_0 .. q_{k-1} mod q_i and ginv[i] = (q_0 .. q_{i-1})^-1 mod q_i;
// half[i] are the mixed-radix digits of floor(Q0 / 2).  The device arrays run
// over the ROOT limbs j of the tables: rad[j][i] = q_0 .. q_{i-1} mod q_j and
// its Shoup companion ([L][kRaiseMax]), q0m[j] = Q0 mod q_j.
constexpr size_t kRaiseMax = 4;
struct RaiseDigits {
  uint64_t pre[kRaiseMax][kRaiseMax], prep[kRaiseMax][kRaiseMax];
  uint64_t ginv[kRaiseMax], ginvp[kRaiseMax];
  uint64_t half[kRaiseMax];
};
struct RaiseConsts {
  RaiseDigits g{};
  const void* rad = nullptr;
  const void* radp = nullptr;
  const void* q0m = nullptr;
};
struct RaiseDev {
  size_t l0 = 0;
  void* dev = nullptr;
  RaiseConsts rc{};
};

struct Tables {
  int device = 0;
  int wide = 0;            // 0: W = u32, 1: W = u64
  bool lazy30 = false;     // every modulus < 2^30: Harvey-lazy product path (u32)
  bool lazy62 = false;     // u64 words, every modulus < 2^62: the same for u64
  bool ks_diag = true;     // ct-mul key-switch diagonal from the tensor's d2^ (RNT_KS_DIAG)
  int rot_fuse = 1;        // rotation: sigma(c0) gathered by the key-switch inverse (RNT_ROT_FUSE: 1 one ct, 2 any, 0 off)
  int plane = 0;           // the whole-plane kernels where they apply (plane_ok, mf_ok);
  int mf_mul = 1;          // rnt_mul at N = 2^16 on the matrix-core transforms (RNT_MF_MUL=0: k_plane_fused)
                           // RNT_PLANE=0: the four-step kernels everywhere
  uint32_t dec_jg = 0;     // key-switch decomposition: target limbs per workgroup (0 = auto)
  size_t ks_ws_bytes = (size_t)4096 << 20;  // key-switch scratch cap per chunk (RNT_KS_WS_MB)
  int md_auto = 1;         // the tail of a hoisted hybrid rotation (RNT_MODDOWN_AUTO): 1 k_moddown_auto where
                           // a chunk's component is below kMdAutoBytes, else k_moddown, the automorphism
                           // launch and a strided copy; 0 never k_moddown_auto, 2 always (A/B, tests)
  uint32_t log_n = 0;
  size_t n = 0;
  size_t L = 0;            // channel count of the root basis
  std::vector<uint64_t> moduli;
  std::vector<uint64_t> psi;
  void* tw_fwd = nullptr;   // [L][N] Tw<W>{psi^{brv(g)}, companion}, heap order g in [1, N)
  void* tw_inv = nullptr;   // [L][N] Tw<W>{psi^{-brv(g)}, companion}
  void* lconst = nullptr;   // [L] LimbConst<W>
  void* resc = nullptr;     // [L][L]: resc[l][i] = (q_l mod q_i)^-1 mod q_i, i < l
  void* resc_p = nullptr;   // [L][L] Shoup companions
  hipStream_t stream = nullptr;      // where every op is queued (rnt_ctx_set_stream)
  hipStream_t own_stream = nullptr;  // created with the context
  // rnt_rescale_ext constants per external last modulus: device arrays
  // {inv[L], invp[L]} with inv[l] = (q_last mod q_l)^-1 mod q_l.
  std::mutex resc_mu;
  std::vector<std::pair<uint64_t, void*>> resc_ext;
  // centred-CRT constants per limb count (rnt_to_coeffs / rnt_crt_centered)
  std::vector<std::pair<size_t, struct CrtDev>> crt_cache;
  // hybrid key-switch constants (rnt_*_hybrid) of a key basis, per (key limbs,
  // ciphertext limbs, alpha, limb map); under resc_mu, built on first use
  std::vector<struct HybridDev> hyb_cache;
  // rnt_mod_raise constants per input limb count (under resc_mu, built on first use)
  std::vector<struct RaiseDev> raise_cache;
  // CKKS special-FFT twiddles (rnt_encode.hip), [N/2] double2, built on
  // first encode/decode
  std::mutex sfft_mu;
  void* sfft_tw = nullptr;
  struct Prof* prof = nullptr;  // per-kernel event timing (rnt_profile_*)
  // MFMA transform tables (rnt_mfma.hip: matrix operands, compensations and
  // twists per limb), built by rnt_ctx_create where mf_supported()
  void* mf = nullptr;
  ~Tables();
};

// Kernel ids for rnt_profile_read.
enum KernelId {
  K_COL_FWD, K_ROW_FWD, K_ROW_INV, K_ROW_MUL, K_COL_INV, K_ELEMENTWISE, K_RESCALE,
  K_AUTOMORPHISM, K_KS_DECOMPOSE, K_KS_ROWS, K_TENSOR_ROWS, K_IMPORT, K_EXPORT, K_CRT,
  K_SFFT, K_SAMPLE, K_COPY, K_PLANE_FUSED, K_MF_NTT_FWD, K_MF_NTT_INV, K_WHOLE_FWD, K_WHOLE_INV, K_WHOLE_MUL,
  K_KS_WHOLE, K_TENSOR_WHOLE, K_MF_TENSOR, K_MF_MUL, K_BSGS_MAC, K_HOIST_DIGITS, K_HOIST_MAC, K_MODUP, K_MODDOWN,
  K_MODDOWN_AUTO, K_MODDOWN_RESCALE, K_LINCOMB, K_DOT_TENSOR, K_MOD_RAISE, K_MUL_MONOMIAL,
  K_MODDOWN_RESCALE_AFFINE, K_DH_BSGS_MAC, K_DH_BSGS_FOLD, K_ROTSUM_MAC, K_ROTSUM_C0, K_AUTOMORPH_NTT, K_PLAIN_MAC, K_COUNT
};

struct Prof {
  std::mutex mu;
  bool on = false;
  struct Rec {
    int id;
    hipEvent_t a, b;
  };
  std::vector<Rec> pending;
  std::vector<hipEvent_t> pool;
  uint64_t launches[K_COUNT] = {};
  double ms[K_COUNT] = {};
  // the first failure of a profiling call (event create / record / elapsed
  // time): profiling turns itself off and rnt_profile_read reports it; it
  // never aborts or fails a launch
  hipError_t err = hipSuccess;
  const char* err_where = nullptr;
};

}  // namespace rnt

// Arc<RnsBasis> semantics: a context lives until rnt_ctx_destroy has been
// called AND every buffer allocated on it has been freed, so handles may be
// released in any order (e.g. by a garbage collector).
struct rnt_ctx {
  std::shared_ptr<rnt::Tables> t;
  size_t L = 0;  // channel count of this (possibly dropped) basis
  std::atomic<long> refs{1};  // 1 for the creator + 1 per live buffer
  // A level context (rnt_ctx_hybrid_level): the basis q_0..q_{level-1},
  // p_0..p_{K-1} of `parent` (retained), L = level + K.  Working limb t is the
  // tables' limb t below `level` and t + gap from there on.  It holds key
  // views alone (rnt_key_level_view): nothing is allocated on it.
  const rnt_ctx* parent = nullptr;
  size_t level = 0, gap = 0;
  bool is_level() const { return parent != nullptr; }
  size_t root_limb(size_t t) const { return parent && t >= level ? t + gap : t; }
  uint64_t modulus(size_t t) const { return this->t->moduli[root_limb(t)]; }
};

struct rnt_buf {
  const rnt_ctx* ctx = nullptr;
  size_t n_polys = 0;
  void* data = nullptr;       // [L][B][N] words
  size_t data_bytes = 0;      // size of the block holding `data` (owned buffers)
  int in_ntt = 0;
  // lazily grown per-buffer workspace (buffers are never used by two
  // threads at once, so this needs no lock)
  void* ws = nullptr;
  size_t ws_bytes = 0;
  void* stage = nullptr;      // u64 host-format staging for upload/download
  size_t stage_bytes = 0;
  bool owns = true;           // false: rnt_buf_wrap view of caller memory
  // A key level view (rnt_key_level_view; ctx is a level context, owns false,
  // data the parent's): logical poly g beta' + d on working limb t is the
  // parent's plane (ctx->root_limb(t) stored_polys + g step_polys + d) N.
  const rnt_buf* view_of = nullptr;
  size_t stored_polys = 0;    // the parent's polys: its limb stride in planes
  size_t step_polys = 0;      // the full key's digits beta: the poly stride of a set's steps
};

namespace rnt {

// Geometry of the N = R * C split.
struct Geom {
  uint32_t log_n, log_r, log_c;
  size_t n, r, c;
};
Geom geom_for(uint32_t log_n);

// Kernel argument bundle common to all launches.
struct Launch {
  const Tables* t;
  size_t L;            // limbs processed (prefix of the root basis)
  size_t B;            // polys per buffer
  hipStream_t s;
  size_t Ls = 0;       // key-switch source limbs (0: same as L)
  // The ct-mul key-switch's diagonal (source limb i == target limb i, the
  // same basis): the tensor launches write the exact d2^ here ([L][B][N],
  // limb stride d2hat_ls), the decomposition skips those planes and the
  // key-switch rows read them instead of transforming S (nullptr: off)
  void* d2hat = nullptr;
  uint64_t d2hat_ls = 0;
  // The rotation's sigma_g(c0) read straight from c0 by the key-switch
  // inverse's addend (g^-1 mod 2N, odd; 0: the addend as it is): no
  // separate automorphism launch for c0 (tiled column grids only)
  uint32_t add_ginv = 0;
  // The transforms' table-limb base: limb l of the launch reads the tables of
  // root limb tab0 + l (the forward / inverse transforms alone: col_fwd, row,
  // whole modes 0 / 1, col_inv without ColRescArgs, mf_ntt).  The data pointer
  // is the launch's first limb.
  uint32_t tab0 = 0;
  // The limb map of a hybrid key's level view (the hybrid kernels alone):
  // working limb t is root limb t below map_level, t + map_gap from there on.
  uint32_t map_level = UINT32_MAX;
  uint32_t map_gap = 0;
  size_t src_limbs() const { return Ls ? Ls : L; }
};

// ---- launchers (one per kernel family, beside its kernels), W-dispatched by t->wide
// All arrays are [limb][poly][N] with an explicit limb stride `*_ls` (words);
// k.B polys (a batch or a chunk of one) and k.L limbs are processed.
// Forward column pass on up to two operands (in0->out0, in1->out1).
// lazy (all three): the product path's Harvey-lazy 30-bit variant (q < 2^30,
// see rnt_modarith.hpp Mod30) where lazy_ok(); the intermediates between
// the three launches are then unreduced, the product's output canonical.
bool lazy_ok(const Tables* t);
hipError_t launch_col_fwd(const Launch& k, void* out0, const void* in0, void* out1,
                          const void* in1, uint64_t in_ls, uint64_t out_ls, bool lazy = false);
// Row pass.  mode 0: forward rows (in place on x); 1: inverse rows (in place
// on x); 2: poly-mul rows: x <- INVrow(FWDrow(x) (.) FWDrow(y) * 2^-w).
hipError_t launch_row(const Launch& k, int mode, void* x, const void* y, uint64_t ls,
                      bool lazy = false);
// The whole-plane product for u32 canonical bases at N = 2^16 (rnt_plane.hip;
// 5 planes of HBM traffic per (poly, limb) instead of the four-step path's
// 9): out = a * b in the coefficient domain (out may alias a or b; scratch:
// one word per output word, a^ in a private layout).
bool plane_ok(const Tables* t);
hipError_t launch_plane_fused(const Launch& k, void* out, const void* a, const void* b, void* scratch, uint64_t ls);
// Scratch slots indexed by the CU a 160-KiB-LDS workgroup runs on (XCC_ID
// and HW_ID bits 15..8): k_plane_fused_slots, k_mf_tensor from this many
// (poly, limb) pairs on.
constexpr uint32_t kPlaneSlots = 1u << 11;
// scratch planes (of N words) launch_plane_fused needs for B L pairs
uint64_t plane_scratch_planes(uint64_t planes);
// The standalone transforms at the same size (rnt_mfma.hip): radix-16 passes
// as i8 matrix products, in place.  mf_supported: u32 bases at N = 2^16;
// mf_build: the per-limb tables into t->mf (0 ok, else err).
inline bool mf_supported(const Tables* t) { return t->plane != 0 && !t->wide && t->log_n == 16; }
int mf_build(Tables* t, std::string* err);
hipError_t launch_mf_ntt(const Launch& k, int inverse, void* data, uint64_t ls);
// The ciphertext tensor product at N = 2^16 on the matrix-core transforms
// (k_mf_tensor, mf_supported bases): coefficient-domain c0, c1, c0', c1' at
// limb stride ils -> NTT-domain d0^, d1^ (Montgomery-scaled key-switch seeds)
// and coefficient-domain d2 at limb stride ols; scratch: plane_scratch_planes(B L)
// planes of N words.
hipError_t launch_mf_tensor(const Launch& k, void* d0, void* d1, void* d2, uint64_t ols, const void* c0,
                            const void* c1, const void* c0p, const void* c1p, uint64_t ils, void* scratch);
// The coefficient-domain product c = a b at N = 2^16 on the matrix-core
// transforms (k_mf_mul, mf_supported bases; in place allowed); scratch:
// plane_scratch_planes(B L) planes of N words.
hipError_t launch_mf_mul(const Launch& k, void* c, const void* a, const void* b, uint64_t ls, void* scratch);
// Whether rnt_mul's row kernel stops its transforms two stages early and
// multiplies degree-3 residues (u32 canonical bases, row length 2^(4k));
// its inverse column pass then takes rfold = 2.
bool mul_truncated(const Tables* t);
// The whole-plane row path at 2^10 <= N <= 2^14 (u32 and u64; rnt_rows.hip
// k_row<..., WHOLE>): one launch per transform or product, every plane one
// row.  mode 0: forward in place (x); 1: inverse in place (x); 2: out = x * y
// in the coefficient domain (out may alias x or y).  whole_ok: the path serves
// this mode on this basis.
bool whole_ok(const Tables* t, int mode);
hipError_t launch_whole(const Launch& k, int mode, void* out, void* x, const void* y, uint64_t ls);
// Inverse column pass with n^-1 folded into the last stage; rfold adds the
// Montgomery factor 2^w.  addend (optional, coefficient domain, out layout).
// ColRescArgs (tiled grids, log R >= 5, col_resc_ok): limb0 offsets the
// launch's limbs in the basis' tables (in/out point at the first one); with
// `last` ([B][N], the dropped limb's coefficient plane) the output is
// rescaled: (c_l - (c_last mod q_l)) inv[l], inv/invp the rows
// resc_inv_row(t, last limb, 0 / 1) of the rescale table.
struct ColRescArgs {
  const void* last = nullptr;
  const void* inv = nullptr;
  const void* invp = nullptr;
  uint32_t limb0 = 0;
};
hipError_t launch_col_inv(const Launch& k, void* out, uint64_t out_ls, const void* in,
                          uint64_t in_ls, int rfold, const void* addend, bool lazy = false,
                          const ColRescArgs& ra = ColRescArgs{});
bool col_resc_ok(const Tables* t);
const void* resc_inv_row(const Tables* t, size_t last, int which);
// Elementwise over k.L*k.B*N contiguous words: op 0 add, 1 sub, 2 neg,
// 3 pointwise mul (canonical a*b mod q), 4 Montgomery product (a*b*2^-w).
hipError_t launch_elementwise(const Launch& k, int op, void* out, const void* a,
                              const void* b);
// Plain device copy of `bytes` (16-byte aligned pointers, bytes % 16 == 0):
// every lane moves 4 x 16 B, loads before stores (Clone, rnt_copy).
hipError_t launch_copy(hipStream_t s, void* dst, const void* src, uint64_t bytes);
// `rows` runs of run_bytes bytes in one launch (k_copy_rows), row r at + r
// pitch on either side; everything a multiple of 4 bytes, 16-byte accesses
// where everything is a multiple of 16.  dst and src do not overlap.
hipError_t launch_copy_rows(hipStream_t s, void* dst, uint64_t dst_pitch_bytes, const void* src,
                            uint64_t src_pitch_bytes, uint64_t run_bytes, size_t rows);
// k.L = limbs of the input; output has k.L - 1 (same poly count / stride B*N).
hipError_t launch_rescale(const Launch& k, void* out, const void* in);
// Centred CRT of every coefficient (coefficient-domain `in`, k.L limbs) into
// `out_words` 64-bit two's-complement words each ([B][N][out_words]);
// `consts` points to a host CrtConsts of device arrays, mw = 32-bit words of Q.
hipError_t launch_crt(const Launch& k, uint64_t* out, const void* in, const void* consts,
                      uint32_t mw, uint32_t out_words);
// out limb l = (in_l - (last mod q_l)) * inv[l] (Shoup pair inv/invp, device
// arrays of k.L words); `last` is a [B][N] plane of residues mod q_last.
hipError_t launch_rescale_ext(const Launch& k, void* out, const void* in, const void* last,
                              const void* inv, const void* invp);
hipError_t launch_automorphism(const Launch& k, void* out, const void* in, uint64_t g);
// host u64 [B][L][N] staging <-> device; err_index receives the smallest
// offending flat index (UINT64_MAX if none) for non-reduced input.
hipError_t launch_import(const Launch& k, void* dst, const uint64_t* stage, int to_brv,
                         unsigned long long* err_index);
hipError_t launch_import_coeffs(const Launch& k, void* dst, const int64_t* stage);
// k.B polys starting at src; ls = limb stride in words (0: k.B * N)
hipError_t launch_export(const Launch& k, uint64_t* stage, const void* src, int from_brv,
                         uint64_t ls = 0);
// Key-switch pieces.  S: [L_target][L_source][k.B][N] scratch (chunk-local).
hipError_t launch_ks_decompose(const Launch& k, void* S, const void* d, uint64_t d_ls);
// u0 rows <- INVrow(sum_i FWDrow(S[j][i]) (.) key_b[i][j] (+ init0)), u1 with
// key_a.  init0/init1 may be null (NTT-domain rows, Montgomery-scaled).
hipError_t launch_ks_rows(const Launch& k, void* u0, void* u1, uint64_t u_ls, const void* S,
                          const void* key_a, const void* key_b, uint64_t key_ls,
                          const void* init0, const void* init1, uint64_t init_ls);
// The same for one term of rnt_ct_linear (k_ks_rows<..., LIN>): both sums are
// multiplied by the plaintext row `mul` (one [N] plane per limb at limb stride
// mul_ls, Montgomery form m^ 2^w mod q, shared by every poly) before the
// inverse rows, which are added to u0/u1 when `accum` is set (stored otherwise).
struct KsLin {
  const void* mul = nullptr;
  uint64_t mul_ls = 0;
  uint32_t accum = 0;
};
hipError_t launch_ks_rows_lin(const Launch& k, void* u0, void* u1, uint64_t u_ls, const void* S,
                              const void* key_a, const void* key_b, uint64_t key_ls,
                              const void* init0, const void* init1, uint64_t init_ls, const KsLin& lin);
// Pointwise products over k.L x k.B x N contiguous words (k_bcast_mul).
// kind 0: out = x (.) m 2^-w, m one [N] plane per limb at limb stride m_ls
// broadcast over the batch (m null: out = x 2^-w), added to out with accum;
// kind 1: out = x 2^w mod q (canonical -> Montgomery form).  out may be x.
hipError_t launch_bcast_mul(const Launch& k, int kind, void* out, const void* x, const void* m,
                            uint64_t m_ls, bool accum);
// The inner sums of rnt_ct_linear_bsgs (k_bsgs_mac), both components of nj <=
// kBsgsJt giant steps in one launch: outs[jj] + comp blk_words = sum_b
// x[2 b + comp] (.) m[jj n_baby + b] (+ the words already there with bit jj of
// accum_mask), b < n_baby, comp in {0, 1}.  x is 2 n_baby NTT-domain blocks of
// blk_words words, each [k.L][k.B][N]; m points at plane (jj = 0, b = 0) of
// the Montgomery-form plaintexts, one [N] plane per limb and pair at limb
// stride m_ls, broadcast over the batch.  The outputs are distinct from x.
constexpr uint32_t kBsgsJt = 4;
hipError_t launch_bsgs_mac(const Launch& k, void* const* outs, uint32_t nj, uint32_t accum_mask,
                           const void* x, uint64_t blk_words, const void* m, uint64_t m_ls,
                           uint32_t n_baby);
// The hoisted rotations (rnt_ct_rotate_hoisted).  launch_hoist_digits
// (k_hoist_digits): D[j][i][p] = (limb i, poly p of c1) 2^w mod q_j for j < k.L,
// i < k.src_limbs(), p < k.B; c1 coefficient-domain at limb stride src_ls, D
// [k.L][k.src_limbs()][k.B][N], to be transformed forward as a buffer of k.L
// limbs and src_limbs k.B polys.  launch_hoist_mac (k_hoist_mac), nt <= kHoistT
// steps in one launch: acc0[t] = sum_i D^[j][i] (.) key_b[t][i][j], acc1[t] with
// key_a ([k.L][k.B][N] each, NTT domain, canonical); key_*[t] points at step t's
// hoisting-form key (source limb i at + i N words, limb j at + j key_ls).
constexpr uint32_t kHoistT = 4;
hipError_t launch_hoist_digits(const Launch& k, void* D, const void* c1, uint64_t src_ls);
hipError_t launch_hoist_mac(const Launch& k, void* const* acc0, void* const* acc1, uint32_t nt, const void* d,
                            const void* const* key_a, const void* const* key_b, uint64_t key_ls);
// The same sums ADDED to what acc0[t] / acc1[t] hold (k_hoist_mac_acc): the
// giant stage of rnt_ct_linear_bsgs_hybrid, one A0 / A1 over several launches.
hipError_t launch_hoist_mac_acc(const Launch& k, void* const* acc0, void* const* acc1, uint32_t nt, const void* d,
                                const void* const* key_a, const void* const* key_b, uint64_t key_ls);
// The automorphism in the NTT domain and the rotate-and-sum built on it
// (rnt_automorphism_ntt, rnt_ct_rotsum_hybrid).  launch_automorphism_ntt
// (k_automorph_ntt): out = the NTT-domain words of sigma_g(in), g odd, out not
// in.  launch_rotsum_mac (k_rotsum_mac), nt <= kRotsumT steps in one launch:
// acc0 (+)= sum_t sum_d sigma_{g[t]}(D^[j][d]) (.) key_b[t][d][j], acc1 with
// key_a; D the block launch_modup wrote, transformed (k.src_limbs() = beta);
// key_*[t] points at step t's ORDINARY key (digit d at + d N words, limb j at
// + j key_ls), read through the limb map; accum: added to what acc0 / acc1
// hold.  launch_rotsum_c0 (k_rotsum_c0): out = z x + sum_{t < nt} sigma_{g[t]}(x)
// in the coefficient domain over k.L limbs, x at limb stride x_ls, out at the
// chunk's own; accum: added to out.
constexpr uint32_t kRotsumT = 8;
hipError_t launch_automorphism_ntt(const Launch& k, void* out, const void* in, uint64_t g);
hipError_t launch_rotsum_mac(const Launch& k, void* acc0, void* acc1, uint32_t nt, const uint64_t* g, const void* d,
                             const void* const* key_a, const void* const* key_b, uint64_t key_ls, bool accum);
hipError_t launch_rotsum_c0(const Launch& k, void* out, const void* x, uint64_t x_ls, uint32_t nt, const uint64_t* g,
                            uint32_t z, bool accum);
// Hybrid key-switching (rnt_keyswitch_hybrid).  k.t is the KEY basis' tables,
// k.L = Lv + K its limbs, k.B the chunk's polys.  These launchers and the three
// launch_hoist_mac* read the limb constants and the key planes through the limb
// map (k.map_level, k.map_gap: a key level view); D, A and the constants of hc
// stay dense in working limbs.  launch_modup (k_modup): the
// Montgomery-form raised digits D[t][d][p] = ModUp_d(x) 2^w mod m_t for t < k.L,
// d < hc.beta, x coefficient-domain over the first Lv limbs at limb stride
// src_ls; D is [k.L][beta][k.B][N], the block launch_hoist_mac reads with
// Ls = beta.  launch_moddown (k_moddown): out_j = (A_j - conv_j) P^-1 (+ add_j)
// for j < Lv from the coefficient-domain A ([k.L][k.B][N] at limb stride a_ls);
// out at limb stride out_ls, the optional addend at add_ls.
hipError_t launch_modup(const Launch& k, void* D, const void* x, uint64_t src_ls, const HybridConsts& hc);
hipError_t launch_moddown(const Launch& k, void* out, uint64_t out_ls, const void* A, uint64_t a_ls,
                          const void* add, uint64_t add_ls, const HybridConsts& hc);
// launch_moddown_auto (k_moddown_auto): sigma_g of launch_moddown's result (g
// odd, below 2N), scattered at the output's limb stride; out overlaps neither
// A nor the addend.
hipError_t launch_moddown_auto(const Launch& k, void* out, uint64_t out_ls, const void* A, uint64_t a_ls,
                               const void* add, uint64_t add_ls, uint64_t g, const HybridConsts& hc);
// launch_moddown_rescale (k_moddown_rescale): launch_moddown's result rescaled
// by its last limb without reaching memory -- out_j = (r_j - [r_{Lv-1}]_{q_j})
// rinv[j] for j < Lv - 1, r = ModDown(A) (+ add); rinv / rinvp are the row
// resc_inv_row(ciphertext tables, Lv - 1, 0 / 1) launch_rescale reads.  The
// words are those of launch_moddown followed by launch_rescale.  Lv >= 2.
// MdAffine (on): the kernel's affine epilogue, out_j = w o_j + u z_j (+ bias on
// coefficient 0 of every poly) mod q_j with o the rescaled result; z (optional,
// coefficient domain, Lv - 1 limbs at limb stride z_ls) may be `out`.  The
// three integers go to the kernel by value: no table, no host copy.
struct MdAffine {
  bool on = false;
  int64_t w = 1, u = 0, bias = 0;
  const void* z = nullptr;
  uint64_t z_ls = 0;
};
hipError_t launch_moddown_rescale(const Launch& k, void* out, uint64_t out_ls, const void* A, uint64_t a_ls,
                                  const void* add, uint64_t add_ls, const void* rinv, const void* rinvp,
                                  const HybridConsts& hc, const MdAffine& af = MdAffine{});
// launch_lincomb (k_lincomb): n_out scalar linear combinations of n_in
// ciphertexts, both components in one launch.  k.L = Lv limbs of the inputs,
// k.B ciphertexts; x0 / x1 hold n_in k.B polys a limb at limb stride in_ls
// (term i at poly i k.B), out0 / out1 n_out k.B at out_ls over Lv limbs, or
// Lv - 1 with `rescale` (the words of launch_rescale on the sums, which are not
// written; Lv >= 2).  w / wp: device [Lv][n_out][n_in] weights mod q_t and
// their Shoup companions; bias: device [Lv][n_out] (coefficient 0 of component
// 0) or nullptr.  1 <= n_in, n_out <= kLincombMax.
constexpr size_t kLincombMax = 16;
hipError_t launch_lincomb(const Launch& k, void* out0, void* out1, uint64_t out_ls, const void* x0, const void* x1,
                          uint64_t in_ls, size_t n_in, size_t n_out, const void* w, const void* wp, const void* bias,
                          bool rescale);
// launch_dot_tensor (k_dot_tensor): the tensor sums of nt <= kDotT terms of a
// ciphertext inner product.  k.L = Lv limbs, k.B = the chunk's ciphertexts;
// x0 / x1 / y0 / y1: NTT-domain planes at limb stride in_ls, term i at
// + i term_words of a limb; d0 / d1 / d2: sum_i x0_i y0_i, sum_i (x0_i y1_i +
// x1_i y0_i), sum_i x1_i y1_i, each times 2^-w, at limb stride out_ls -- added
// to the words already there with `accum`.  y0 == x0 with y1 == x1 takes the
// squares form (two loads a term).  The outputs alias no input.
constexpr size_t kDotT = 4;
hipError_t launch_dot_tensor(const Launch& k, void* d0, void* d1, void* d2, uint64_t out_ls, const void* x0,
                             const void* x1, const void* y0, const void* y1, uint64_t in_ls, uint64_t term_words,
                             size_t nt, bool accum);
// launch_plain_mac (k_plain_mac): the plaintext sums of nt <= kPlainT terms of
// rnt_ct_plain_mac.  k.L = Lv limbs, k.B = the chunk's ciphertexts; x0 / x1:
// NTT-domain planes at limb stride in_ls, term i at + i term_words of a limb;
// m: the NTT-domain plaintexts at limb stride m_ls, term i at + i m_term_words,
// one plane for every ciphertext (m_shared) or k.B planes; bias: nullptr, or
// NTT-domain words at limb stride b_ls, one plane (b_shared) or k.B.  d0 / d1:
// sum_i x0_i m_i (+ bias) and sum_i x1_i m_i, canonical, at limb stride out_ls
// -- added to the words already there with `accum`.  The outputs alias no input.
// kPlainT: the largest of 4, 8, 16 at which every form of the kernel keeps 0
// bytes of scratch and the occupancy of k_dot_tensor's same form (DESIGN.md §4
// "rnt_ct_plain_mac").
constexpr size_t kPlainT = 16;
hipError_t launch_plain_mac(const Launch& k, void* d0, void* d1, uint64_t out_ls, const void* x0, const void* x1,
                            uint64_t in_ls, uint64_t term_words, const void* m, uint64_t m_ls, uint64_t m_term_words,
                            bool m_shared, const void* bias, uint64_t b_ls, bool b_shared, size_t nt, bool accum);
// launch_mod_raise (rnt_raise.hip k_mod_raise): k.t the OUTPUT basis' tables,
// k.L its limbs, k.B polys; `in` holds l0 < k.L coefficient-domain limbs of k.B
// polys (limb stride k.B N, as `out`) whose moduli are the tables' first l0.
// Limb j of out = (the centred CRT value of in) mod q_j, canonical.
hipError_t launch_mod_raise(const Launch& k, void* out, const void* in, size_t l0, const RaiseConsts& rc);
// launch_mul_monomial (k_mul_monomial): out = in X^shift over k.L x k.B x N
// contiguous words, shift in [0, 2N); out and in do not overlap.
hipError_t launch_mul_monomial(const Launch& k, void* out, const void* in, uint64_t shift);
// launch_hoist_mac_seed (k_hoist_mac_seed): launch_hoist_mac for one step whose
// sums start, on the limbs j < hc.Lv, from seed_b[j] (P 2^w mod q_j) and
// seed_a[j] (P 2^w mod q_j) and from 0 on the special limbs; the seeds are
// NTT-domain d^ 2^-w over the ciphertext limbs at limb stride seed_ls, so the
// accumulators are those of A + P d.
hipError_t launch_hoist_mac_seed(const Launch& k, void* acc0, void* acc1, const void* d, const void* key_a,
                                 const void* key_b, uint64_t key_ls, const void* seed_a, const void* seed_b,
                                 uint64_t seed_ls, const HybridConsts& hc);
// The double-hoisted transform (rnt_ct_linear_bsgs_hybrid_dh).  k as the hybrid
// launchers': the key basis' tables and limb map, k.L = Lv + K, k.B the chunk's
// polys.  launch_dh_bsgs_mac (k_dh_bsgs_mac), nj <= kDhJt giants and nb <= kDhBt
// babies in one launch: out0[jj] (+)= sum_b m[jj][b] (.) sigma_{g[b]}(T0_b + P c0^),
// out1[jj] with T1_b, every block [k.L][k.B][N] in the NTT domain, canonical.
// t0[b] / t1[b]: baby b's hoisted key products over E (launch_hoist_mac's), or
// both nullptr for a step of 0 -- then the term is (P c0^, P c1^) at the lane's
// own position and g[b] is not read.  c0h / c1h: the transformed ciphertext,
// [hc.Lv][k.B][N]; m: plane (jj = 0, b = 0) of the plaintexts over E in plain
// NTT-domain form, dense in working limbs at limb stride m_ls, giant stride
// m_row, baby stride N; accum: added to what the outputs hold.  The outputs
// alias no input.  launch_dh_bsgs_fold (k_dh_bsgs_fold): A0 (+)= sum over the
// nj giants of v0[jj] (g[jj] == 0) or sigma_{g[jj]}(v0[jj]); A1 (+)= the v1[jj]
// with g[jj] == 0; without accum the launch initialises A0 and A1.
constexpr uint32_t kDhJt = 4;
constexpr uint32_t kDhBt = 16;
hipError_t launch_dh_bsgs_mac(const Launch& k, void* const* out0, void* const* out1, uint32_t nj, const void* const* t0,
                              const void* const* t1, const uint64_t* g, uint32_t nb, const void* c0h, const void* c1h,
                              const void* m, uint64_t m_ls, uint64_t m_row, bool accum, const HybridConsts& hc);
hipError_t launch_dh_bsgs_fold(const Launch& k, void* A0, void* A1, const void* const* v0, const void* const* v1,
                               const uint64_t* g, uint32_t nj, bool accum);
// launch_rescale with limb strides: k.B polys of k.L input limbs at in_ls, the
// k.L - 1 output limbs at out_ls (a chunk of a batch on either side).
hipError_t launch_rescale_strided(const Launch& k, void* out, uint64_t out_ls, const void* in, uint64_t in_ls);
// out[l][i] = 2^w mod q_l over [k.L][N]: the Montgomery-form plaintext 1.
hipError_t launch_mont_one(const Launch& k, void* out);
// The whole-plane key-switch at 2^10 <= N <= 2^13 (k_ks_whole, one launch,
// no S): out0 = INV(sum_i NTT(src_i mod q_j) (.) key_b[i][j] + init0) (+ add0),
// out1 likewise with key_a; src is [k.src_limbs()][k.B][N] coefficient-domain
// at limb stride src_ls, out0/out1/add0 at out_ls, init0/init1 (NTT domain,
// Montgomery-scaled, may be null) at init_ls.  ks_whole_ok: it serves this basis.
bool ks_whole_ok(const Tables* t);
hipError_t launch_ks_whole(const Launch& k, void* out0, void* out1, uint64_t out_ls, const void* src,
                           uint64_t src_ls, const void* key_a, const void* key_b, uint64_t key_ls,
                           const void* init0, const void* init1, uint64_t init_ls, const void* add0);
// Tensor rows for ct x ct: inputs are column-transformed c0,c1,c0p,c1p.
// Writes d0hat, d1hat (NTT rows, Montgomery-scaled) and the inverse-row
// output of d2 into d2row.  All arrays share limb stride ls.
// The whole-plane tensor (k_tensor_rows<..., WHOLE>, 2^10 <= N <= 2^13;
// u64 bases N <= 2^12): coefficient-domain c0, c1, c0', c1' -> NTT-domain
// d0^, d1^ and coefficient-domain d2 in one launch.
bool tensor_whole_ok(const Tables* t);
hipError_t launch_tensor_whole(const Launch& k, void* d0hat, void* d1hat, void* d2, uint64_t ls,
                               const void* c0, const void* c1, const void* c0p, const void* c1p,
                               uint64_t in_ls);
hipError_t launch_tensor_rows(const Launch& k, void* d0hat, void* d1hat, void* d2row,
                              const void* c0, const void* c1, const void* c0p,
                              const void* c1p, uint64_t ls);
// Device samplers (rnt_sample.hip): kind 0 uniform residues, 1 rounded
// Gaussian (sigma), 2 ternary with exactly `hamming_weight` nonzeros; every
// poly of `out` ([k.L][k.B][N], limb stride k.B * N) in the coefficient domain.
struct SampleKey {
  uint32_t k0, k1;  // Philox key: seed low word, seed high word ^ stream high word
  uint32_t stream;  // stream low word (a counter word)
};
hipError_t launch_sample(const Launch& k, int kind, void* out, SampleKey s, double sigma,
                         uint32_t hamming_weight);
// CKKS canonical embedding (rnt_encode.hip).  Twiddle table: N/2 complex
// doubles (interleaved re, im).  encode: values [B][n_values] double2 ->
// coeffs [B][N] i64 (work: [B][N/2] double2); decode: centred i64 coeffs
// [B][N] -> work [B][N/2] double2 slots / 2^scale_bits.
bool sfft_supported(uint32_t log_n);
std::vector<double> sfft_twiddles(uint32_t log_n);
hipError_t launch_sfft_encode(const Launch& k, int64_t* coeffs, void* work, const void* values,
                              uint32_t n_values, uint32_t scale_bits, const void* tw);
hipError_t launch_sfft_decode(const Launch& k, void* work, const int64_t* coeffs,
                              uint32_t scale_bits, const void* tw);

}  // namespace rnt
