/*
 * rnsntt.h -- C-ABI of the MI355X-native RNS-NTT backend (librnsntt.so).
 *
 * Drop-in boundary for oiwn/toy-heaan-ckks's `RnsPoly<N>` / `RnsBasis<N>`
 * (src/rings/backends/rns_ntt/) and the key-switch / rescale loops of
 * `CkksEngine` (src/crypto/engine.rs).  Each entry point names the reference
 * interface it replaces (paths relative to the reference repository root).
 *
 * Conventions
 *  - Every function returns an `int` status: 0 = OK, otherwise one of
 *    RNT_ERR_*.  No exception, abort or panic crosses this boundary.
 *    `rnt_last_error()` returns a thread-local human-readable message for the
 *    last failing call on the calling thread.
 *  - Host polynomial data is exactly the reference's memory: a polynomial is
 *    `Vec<[u64; N]>`, i.e. `uint64_t[L][N]` (limb-major, "channels"); a batch
 *    of B polynomials is `uint64_t[B][L][N]`.  Rust passes
 *    `channels.as_ptr() as *const u64`.
 *  - NTT-domain data crossing the boundary is in the reference's natural
 *    order: index k holds a(psi^(2k+1)) mod q_i (poly.rs:136-148).  The
 *    device-internal order is private.
 *  - Ops are asynchronous on the context's stream; `rnt_sync` waits.
 *    Uploads and downloads are synchronous (they validate / return host
 *    data).
 *  - Threading: a context is immutable after creation and may be shared by
 *    any number of host threads (it is the reference's `Arc<RnsBasis>`).  A
 *    buffer must not be used by two threads at once (the reference's `&mut`).
 */
#ifndef RNSNTT_H
#define RNSNTT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RNT_ABI_VERSION 4

/* Status codes.  1..6 mirror RnsNttError in order
 * (src/rings/backends/rns_ntt/errors.rs:4-20). */
enum {
  RNT_OK = 0,
  RNT_ERR_INVALID_DEGREE = 1,      /* RnsNttError::InvalidDegree          */
  RNT_ERR_EMPTY_BASIS = 2,         /* RnsNttError::EmptyBasis             */
  RNT_ERR_NON_NTT_FRIENDLY = 3,    /* RnsNttError::NonNttFriendlyModulus  */
  RNT_ERR_INVALID_MOD_DROP = 4,    /* RnsNttError::InvalidModDrop         */
  RNT_ERR_CHANNEL_COUNT = 5,       /* RnsNttError::ChannelCountMismatch   */
  RNT_ERR_NON_REDUCED = 6,         /* RnsNttError::NonReducedCoefficient  */
  RNT_ERR_DOMAIN_MISMATCH = 7,     /* reference: debug_assert only (poly.rs:264-267, 292-295) */
  RNT_ERR_BASIS_MISMATCH = 8,      /* reference: debug_assert Arc::ptr_eq (poly.rs:260-263, 288-291) */
  RNT_ERR_DEVICE = 9,              /* HIP runtime error                   */
  RNT_ERR_OUT_OF_MEMORY = 10,
  RNT_ERR_BAD_ARGUMENT = 11,
  /* A valid reference input beyond this backend's capacity (no reference
   * variant: the reference accepts it).  Today only ring degrees above
   * 2^17 (rnt_ctx_create); fields = {degree, max_degree}. */
  RNT_ERR_UNSUPPORTED = 12
};

typedef struct rnt_ctx rnt_ctx; /* == Arc<RnsBasis<N>> (basis.rs:90-94) */
typedef struct rnt_buf rnt_buf; /* == device storage of B RnsPoly (poly.rs:25-30) */

/* ---- library / diagnostics ------------------------------------------- */
int rnt_abi_version(void);
const char* rnt_last_error(void);
const char* rnt_status_string(int status);
/* The RnsNttError fields (src/rings/backends/rns_ntt/errors.rs:4-20) of the
 * calling thread's last failing call, so a binding can rebuild the
 * reference's variant exactly.  Returns that call's status and writes
 *   1 InvalidDegree          fields = {degree, 0}
 *   2 EmptyBasis             fields = {0, 0}
 *   3 NonNttFriendlyModulus  fields = {modulus, degree}
 *   4 InvalidModDrop         fields = {drop_count, channel_count}
 *   5 ChannelCountMismatch   fields = {expected, actual}
 *   6 NonReducedCoefficient  fields = {coefficient, modulus}
 *  12 Unsupported            fields = {degree, max_degree} (no reference variant)
 * and {0, 0} for the statuses 7..11, which have no reference variant.
 * 0 (and {0, 0}) if no call on this thread has failed. */
int rnt_last_error_detail(uint64_t fields[2]);

/* Number of visible HIP devices (0 without a GPU; never fails on CPU-only
 * hosts). */
int rnt_device_count(int* n);

/* ---- per-kernel timing (diagnostics; not thread-safe) ------------------ */
/* When enabled on a context, every kernel the library launches on that
 * context's stream is bracketed by HIP events; rnt_profile_read syncs and
 * returns, for one kernel name ("col_fwd", "row_fwd", "row_inv",
 * "row_mul", "col_inv", "elementwise", "rescale", "automorphism",
 * "ks_decompose", "ks_rows", "tensor_rows", "import", "export", "crt", "sfft",
 * "sample", "copy", "plane_fused", "mf_ntt_fwd", "mf_ntt_inv", "whole_fwd",
 * "whole_inv", "whole_mul", "ks_whole", "tensor_whole", "mf_tensor", "mf_mul",
 * "bsgs_mac", "hoist_digits", "hoist_mac", "modup", "moddown",
 * "moddown_auto", "moddown_rescale", "lincomb", "dot_tensor", "mod_raise",
 * "mul_monomial", "moddown_rescale_affine", "dh_bsgs_mac", "dh_bsgs_fold",
 * "rotsum_mac", "rotsum_c0",
 * "automorph_ntt", "plain_mac"), the launch
 * count and summed device milliseconds since enabling. */
int rnt_profile_enable(const rnt_ctx* ctx, int enable);
int rnt_profile_read(const rnt_ctx* ctx, const char* kernel, uint64_t* launches,
                     double* total_ms);
/* Test hook for the deferred-error path: records a failed cleanup call
 * (HIP error `hip_error`, named "rnt_debug_defer") on the calling thread,
 * as a block leaving the device cache would.  The next launch on the thread
 * reports it as RNT_ERR_DEVICE; free / destroy / trim entry points report
 * only their own cleanup failures and leave it pending. */
int rnt_debug_defer(int hip_error);

/* ---- host-side number theory (no device needed) ----------------------- */
/* is_ntt_friendly_prime (src/math/primes.rs:125-131); writes 0/1. */
int rnt_is_ntt_friendly_prime(uint64_t p, uint64_t degree, int* out);
/* generate_primes (src/math/utils.rs:47-80): `count` descending NTT-friendly
 * primes of exactly `bit_size` bits for `degree`. */
int rnt_generate_primes(uint32_t bit_size, size_t count, uint64_t degree,
                        uint64_t* out);
/* psi of NttTable::new (basis.rs:39-40, find_primitive_root :217-237). */
int rnt_find_psi(uint64_t modulus, uint64_t degree, uint64_t* psi);

/* ---- context == RnsBasis ---------------------------------------------- */
/* RnsBasis::new (basis.rs:97-106) + NttTable::new per modulus (:20-84):
 * validates like the reference (EmptyBasis, then per modulus InvalidDegree
 * for a degree that is not a power of two and NonNttFriendlyModulus), builds
 * the device tables on `device`.  A power-of-two degree above 2^17, which the
 * reference accepts, is RNT_ERR_UNSUPPORTED (this backend's table and grid
 * limit), never InvalidDegree. */
int rnt_ctx_create(uint32_t log_n, const uint64_t* moduli, size_t count,
                   int device, rnt_ctx** out);
/* Releases the caller's handle; like dropping an Arc, the context (and its
 * device tables) stays alive until every buffer allocated on it is freed. */
int rnt_ctx_destroy(rnt_ctx* ctx);
/* RnsBasis::drop_last (basis.rs:121-134): a prefix view sharing the
 * parent's device tables (no table copy). */
int rnt_ctx_drop_last(const rnt_ctx* ctx, size_t drop_count, rnt_ctx** out);
/* The LEVEL CONTEXT of a hybrid key context (see "key level views" below):
 * key_ctx has L + K limbs q_0..q_{L-1}, p_0..p_{K-1} with K = n_special and
 * 1 <= level <= L; *out is the basis q_0..q_{level-1}, p_0..p_{K-1}, sharing
 * key_ctx's tables as rnt_ctx_drop_last does (working limb t is key_ctx's limb
 * t below level, t + (L - level) from there on).  rnt_ctx_degree,
 * _channel_count (= level + K), _moduli, _total_bits, _psi, _stream and
 * _destroy report the view.  It holds key level views alone: on it
 * rnt_ctx_drop_last, rnt_buf_alloc, rnt_buf_alloc_uninit and rnt_buf_wrap ->
 * RNT_ERR_UNSUPPORTED (fields 0, 0).  A null argument, n_special == 0 or >=
 * the limb count, level == 0 or > L, or a key_ctx that is itself a level
 * context -> RNT_ERR_BAD_ARGUMENT. */
int rnt_ctx_hybrid_level(const rnt_ctx* key_ctx, size_t n_special, size_t level, rnt_ctx** out);
int rnt_ctx_degree(const rnt_ctx* ctx, size_t* n);
int rnt_ctx_channel_count(const rnt_ctx* ctx, size_t* count); /* basis.rs:116-118 */
int rnt_ctx_moduli(const rnt_ctx* ctx, uint64_t* out);       /* basis.rs:108-110 */
int rnt_ctx_total_bits(const rnt_ctx* ctx, uint32_t* bits);  /* basis.rs:140-145 */
int rnt_ctx_psi(const rnt_ctx* ctx, size_t limb, uint64_t* psi);
/* The HIP stream (hipStream_t) the context's ops are queued on. */
int rnt_ctx_stream(const rnt_ctx* ctx, void** stream);
/* Queue later ops on the caller's `stream` (a hipStream_t of the context's
 * device; NULL restores the context's own stream), ordered after everything
 * already queued.  Applies to every context sharing the tables (drop_last
 * views).  Call it while no other thread issues ops on those contexts; a
 * caller's stream must outlive the context or be replaced first.  This is
 * SURVEY §8b's per-op stream: set it around the ops that belong on it. */
int rnt_ctx_set_stream(const rnt_ctx* ctx, void* stream);
int rnt_sync(const rnt_ctx* ctx);

/* ---- captured op sequences (hipGraph) --------------------------------- */
/* The reference engine calls one ciphertext at a time
 * (mul_ciphertexts_gadget engine.rs:473-539, rotate_ciphertext :412-463), so
 * a fixed per-ciphertext op sequence is launch-bound.  rnt_capture_begin
 * starts recording every op the calling thread then queues on ctx's stream
 * (any context sharing its tables) into a graph instead of running it;
 * rnt_capture_end instantiates it; rnt_graph_launch replays it, with the
 * same buffers, on the context's current stream.  Record only device ops
 * (no upload, download, rnt_sync or allocation that misses the block cache)
 * and run the sequence once un-recorded first, so its workspaces are cached;
 * the graph keeps the workspace blocks its ops took until
 * rnt_graph_destroy (recorded ops share one call-scoped workspace, so N
 * recorded key-switches keep one block, not N).  Buffers the graph reads
 * and writes must outlive it, and so must their private scratch: while a
 * graph is alive, do not run an op on a larger batch into one of its output
 * buffers (an op that grows a buffer's scratch releases the old block, which
 * the graph's replays still write).  rnt_graph_workspace reports the blocks
 * and bytes the graph holds. */
typedef struct rnt_graph rnt_graph;
int rnt_capture_begin(const rnt_ctx* ctx);
int rnt_capture_end(const rnt_ctx* ctx, rnt_graph** out);
int rnt_graph_launch(rnt_graph* graph);
int rnt_graph_destroy(rnt_graph* graph);
int rnt_graph_workspace(const rnt_graph* graph, size_t* blocks, size_t* bytes);

/* ---- buffers == batches of RnsPoly ------------------------------------ */
/* Allocates device storage for n_polys polynomials over ctx's basis, all
 * zero, coefficient domain (RnsPoly::zero, poly.rs:36-43).  The zeroing is
 * queued on the context's stream (rnt_ctx_stream) like every op: a reader on
 * another stream (e.g. through rnt_buf_device_ptr) must order itself after
 * that stream or call rnt_sync first. */
int rnt_buf_alloc(const rnt_ctx* ctx, size_t n_polys, rnt_buf** out);
/* The same buffer with unspecified contents: for an op's output, which the
 * op overwrites entirely (no zero fill queued; the reference has no such
 * constructor -- RnsPoly::zero is rnt_buf_alloc). */
int rnt_buf_alloc_uninit(const rnt_ctx* ctx, size_t n_polys, rnt_buf** out);
/* Frees without waiting for the device: the buffer's device blocks go to a
 * per-device cache behind an event on the context stream, and a later
 * allocation's stream waits on that event before reusing them. */
int rnt_buf_free(rnt_buf* buf);
/* Returns every idle cached block of `device` (-1: all devices) to the HIP
 * allocator, e.g. before a caller's own allocation that failed is retried;
 * writes the bytes released when freed_bytes is non-NULL.  The cache holds
 * at most RNT_WS_POOL_MB MiB (default 1/8 of the device's memory) idle. */
int rnt_pool_trim(int device, size_t* freed_bytes);
int rnt_buf_n_polys(const rnt_buf* buf, size_t* n);
int rnt_buf_is_ntt(const rnt_buf* buf, int* in_ntt); /* is_ntt_domain, poly.rs:127-129 */
/* RnsPoly::from_channels (poly.rs:73-99) for a batch: host
 * uint64_t[n_polys][channels][N]; `channels` must equal the basis' channel
 * count (else RNT_ERR_CHANNEL_COUNT); every residue must be < q_i (else
 * RNT_ERR_NON_REDUCED).  `in_ntt` != 0: natural-order NTT-domain data. */
int rnt_upload(rnt_buf* buf, const uint64_t* host, size_t n_polys,
               size_t channels, int in_ntt);
/* RnsPoly::from_coeffs (poly.rs:49-67) for a batch: host int64_t[n_polys][N]
 * reduced by rem_euclid per channel; result in coefficient domain. */
int rnt_upload_coeffs(rnt_buf* buf, const int64_t* coeffs, size_t n_polys);
/* RnsPoly::channels (poly.rs:119-121): copies uint64_t[n_polys][L][N] out,
 * in the buffer's current domain (natural order when NTT). */
int rnt_download(const rnt_buf* buf, uint64_t* host, size_t n_polys);
/* channels() of polys [first, first + count) of a batch: uint64_t[count][L][N],
 * in the buffer's current domain (natural order when NTT).  A range outside
 * the batch -> RNT_ERR_BAD_ARGUMENT. */
int rnt_download_polys(const rnt_buf* buf, uint64_t* host, size_t first, size_t count);
int rnt_copy(rnt_buf* dst, const rnt_buf* src); /* Clone */
/* PolyRing::to_coeffs (poly.rs:404-427) for a batch: per coefficient the CRT
 * value centred in (-Q/2, Q/2] (reconstruct_centered_coeff, basis.rs:158-180)
 * as int64_t[n_polys][N] -- the value's low 64 bits in two's complement,
 * exactly the reference's result wherever it is defined (Q < 2^128).  An
 * NTT-domain buffer is converted on a temporary copy; the buffer itself is
 * left as it is.
 * Limits (also of rnt_crt_centered and rnt_decode): Q, the product of the
 * context's moduli, has at most 128 32-bit words (4096 bits); a longer Q, a
 * null `host` or an `n_polys` other than the buffer's ->
 * RNT_ERR_BAD_ARGUMENT.  The context of a longer basis is still created and
 * serves every other call. */
int rnt_to_coeffs(const rnt_buf* buf, int64_t* host, size_t n_polys);
/* The same centred CRT value, in (-Q/2, Q/2], without truncation: `words`
 * 64-bit little-endian two's-complement words per coefficient,
 * uint64_t[n_polys][N][words] (the reference's u128 path
 * cannot represent Q >= 2^128).  1 <= words <= 64, anything else ->
 * RNT_ERR_BAD_ARGUMENT; words past the value's own are its sign extension,
 * fewer words than it needs keep its low ones.  64 words hold any value of
 * the longest Q served (128 32-bit words), sign included. */
int rnt_crt_centered(const rnt_buf* buf, uint64_t* host, size_t n_polys, size_t words);
/* Device-memory interop for multi-GPU pipelines (collectives run by the
 * caller, e.g. RCCL through torch.distributed):
 * rnt_buf_wrap makes a NON-owning buffer over caller device memory laid out
 * [L][n_polys][N] in the context's word width (device-internal order when
 * in_ntt); rnt_buf_device_ptr exposes a buffer's storage and word width.
 * device_ptr must be aligned to that word width (rnt_buf_device_ptr's
 * word_bytes: 4 or 8), else RNT_ERR_BAD_ARGUMENT; no more is asked, and every
 * op accepts such a buffer.  16-byte alignment selects the faster
 * instantiations of the kernels that have two ("Alignment of
 * caller planes").
 * Library writes to that storage (including rnt_buf_alloc's zeroing) are
 * queued on the context's stream: order external reads after it (or call
 * rnt_sync). */
int rnt_buf_wrap(const rnt_ctx* ctx, void* device_ptr, size_t n_polys, int in_ntt,
                 rnt_buf** out);
int rnt_buf_device_ptr(const rnt_buf* buf, void** device_ptr, size_t* word_bytes);

/* ---- ring ops (batched; every poly of the buffers participates) -------- */
/* to_ntt_domain / to_coeff_domain (poly.rs:136-166); no-ops when already
 * in the target domain. */
int rnt_ntt_fwd(rnt_buf* buf);
int rnt_ntt_inv(rnt_buf* buf);
/* MulAssign (poly.rs:277-331) as out = a * b: both NTT -> pointwise, result
 * NTT; both coefficient -> negacyclic product, result coefficient.  Mixed
 * domains -> RNT_ERR_DOMAIN_MISMATCH.  out may alias a or b. */
int rnt_mul(rnt_buf* out, const rnt_buf* a, const rnt_buf* b);
/* AddAssign (poly.rs:254-275) as out = a + b, either domain (must match). */
int rnt_add(rnt_buf* out, const rnt_buf* a, const rnt_buf* b);
int rnt_sub(rnt_buf* out, const rnt_buf* a, const rnt_buf* b);
/* Neg (poly.rs:370-385), either domain. */
int rnt_neg(rnt_buf* out, const rnt_buf* a);
/* rescale_into (poly.rs:187-228): `out` belongs to a context equal to
 * drop_last(1) of `in`'s; result coefficient domain, floor division by the
 * last prime. */
int rnt_rescale(rnt_buf* out, const rnt_buf* in);
/* mod_drop_last (poly.rs:169-177): out (a context equal to drop_last(k) of
 * in's) receives the first L-k channels; domain preserved. */
int rnt_mod_drop_last(rnt_buf* out, const rnt_buf* in);
/* automorphism X -> X^g (poly.rs:492-541). Output coefficient domain, except
 * g mod 2N == 0 which copies `in` (domain preserved) like the reference. */
int rnt_automorphism(rnt_buf* out, const rnt_buf* in, uint64_t g);
/* rotate_slots (poly.rs:546-569): g = 5^k mod 2N (k >= 0); for k < 0 the
 * reference's automorphism(5^|k|) then automorphism(2N-1). */
int rnt_rotate_slots(rnt_buf* out, const rnt_buf* in, int32_t k);
/* The automorphism X -> X^g in the NTT domain (rnt_automorphism_ntt; no
 * reference counterpart): `in` is in the NTT domain, g is odd, and `out` receives the NTT-domain words of
 * sigma_g(in) -- DEFINED as rnt_ntt_fwd(rnt_automorphism(., g)), word for word,
 * but no inverse or forward transform runs: in the NTT domain sigma_g is a pure
 * permutation of the evaluation points, with no sign changes (one gather
 * launch; DESIGN.md "Rotate-and-sum").  g is taken mod 2N.  Both buffers on one
 * context with one batch size; `out` must not alias `in`; recordable.
 * Errors: a coefficient-domain `in` -> RNT_ERR_DOMAIN_MISMATCH; an even g,
 * out == in, batch sizes that differ, a null argument -> RNT_ERR_BAD_ARGUMENT;
 * different contexts -> RNT_ERR_BASIS_MISMATCH; a key level view in any
 * position -> RNT_ERR_UNSUPPORTED (fields 0, 0).  A refused call leaves `out`
 * untouched.  rnt_automorphism itself is unchanged (coefficient-domain
 * output).  Profile name: "automorph_ntt". */
int rnt_automorphism_ntt(rnt_buf* out, const rnt_buf* in, uint64_t g);
/* ModRaise (no reference counterpart): `in` holds B coefficient-domain polys
 * on a context C0 over q_0..q_{l0-1}, 1 <= l0 <= 4; `out` holds B polys on a
 * context C over q_0..q_{L-1}, L > l0, whose first l0 moduli equal C0's BY
 * VALUE -- C0 may be a drop_last view of C, a view of another root or an
 * unrelated root of the same degree, device and device word width.  With x
 * the CRT value of a coefficient's l0 residues centred in (-Q0/2, Q0/2], Q0 =
 * q_0...q_{l0-1} (rnt_crt_centered's convention), limb j of `out` is x mod
 * q_j, canonical; limbs j < l0 are therefore `in`'s words.  `out` is in the
 * coefficient domain.  One launch, l0 planes read and L written, on C's
 * stream (ordered after the work queued on C0's where that is another one).
 * Errors: a null argument, l0 >= L or batch sizes that differ ->
 * RNT_ERR_BAD_ARGUMENT; degree, device or moduli-prefix mismatch ->
 * RNT_ERR_BASIS_MISMATCH; different device word widths, or l0 > 4 ->
 * RNT_ERR_UNSUPPORTED (fields 0, 0); an NTT-domain `in` ->
 * RNT_ERR_DOMAIN_MISMATCH; a key level view in any position ->
 * RNT_ERR_UNSUPPORTED.  A refused call leaves `out` untouched.  The constants
 * of (C's root, l0) are built by the first call that needs them, which
 * therefore CANNOT be recorded (rnt_capture_begin: run the call once first),
 * as for the hybrid calls.  Profile name: "mod_raise". */
int rnt_mod_raise(rnt_buf* out, const rnt_buf* in);
/* out = in * X^k in Z_q[X]/(X^N + 1) for every limb and poly, k taken mod 2N
 * (negative k allowed): with k in [0, 2N), coefficient j of `in` lands at
 * (j + k) mod N, negated when floor((j + k) / N) is odd; canonical (0 stays
 * 0).  Both buffers on one context, coefficient domain; recordable.  out == in
 * -> RNT_ERR_BAD_ARGUMENT (the buffers must not overlap); an NTT-domain `in`
 * -> RNT_ERR_DOMAIN_MISMATCH.  In the CKKS embedding X^(N/2) is i in every
 * slot, so k = N/2 and k = 3N/2 multiply a plaintext's slots by i and -i
 * exactly.  Profile name: "mul_monomial". */
int rnt_mul_monomial(rnt_buf* out, const rnt_buf* in, int64_t k);

/* ---- samplers (PolySampler, src/rings/traits.rs:74-127) */
/* Fill every poly of `out` (coefficient domain) from the counter-based
 * Philox4x32-10 stream (seed, stream): a draw depends only on (seed, stream,
 * sampler, poly, limb, index), never on launch geometry or batch split.  The
 * reference's ChaCha20 streams are not reproduced.
 *   uniform  : residues uniform in [0, q_l), independent per limb
 *              (sample_uniform, poly.rs:438-444);
 *   gaussian : round(N(0, std_dev)) per coefficient, reduced into every limb
 *              (sample_gaussian, poly.rs:447-459); std_dev must be finite > 0;
 *   ternary  : exactly hamming_weight coefficients +-1, the rest 0
 *              (sample_tribits, poly.rs:462-469); hamming_weight <= N. */
int rnt_sample_uniform(rnt_buf* out, uint64_t seed, uint64_t stream);
int rnt_sample_gaussian(rnt_buf* out, double std_dev, uint64_t seed, uint64_t stream);
int rnt_sample_ternary(rnt_buf* out, size_t hamming_weight, uint64_t seed, uint64_t stream);

/* ---- CKKS encoder / decoder (src/encoding) ---------- */
/* CkksEncoder::encode_complex (ckks_encoder.rs:85-122) for every poly of
 * `out`: values = [n_polys][n_values] complex slots as interleaved (re, im)
 * doubles, n_values <= N/2 (zero-padded to N/2, build_conjugate_slots,
 * special_fft.rs:158-178); slots times 2^scale_bits -> the inverse canonical
 * embedding (special_idft, special_fft.rs:194-220, as an O(N log N) special
 * FFT) -> coefficients rounded like f64::round -> residues like from_coeffs
 * (poly.rs:49-67).  `out` becomes coefficient domain.  n_values > N/2 or
 * scale_bits == 0 -> RNT_ERR_BAD_ARGUMENT (the reference panics). */
int rnt_encode(rnt_buf* out, const double* values, size_t n_values, uint32_t scale_bits);
/* CkksEncoder::decode_complex (ckks_encoder.rs:134-156): centred CRT
 * coefficients (to_coeffs, poly.rs:404-427, its i64 result) -> the canonical
 * embedding (special_dft, special_fft.rs:224-242) -> the first n_values
 * slots / 2^scale_bits into values ([n_polys][n_values] (re, im) pairs). */
int rnt_decode(const rnt_buf* in, double* values, size_t n_values, uint32_t scale_bits);

/* ---- engine-level fused ops (src/crypto/engine.rs) -------------------- */
/* A gadget key (RnsGadgetRelinKey / RnsGadgetRotationKey, engine.rs:224-253):
 * key_a and key_b are buffers of one poly per gadget (source) limb i
 * (poly i = a_i / b_i): L polys for rnt_keyswitch, the global limb count for
 * a limb shard's rnt_keyswitch_ext (validated by the key-switch calls).  They
 * are kept device-resident in the NTT domain; rnt_key_prepare transforms
 * them once. */
int rnt_key_prepare(rnt_buf* key_a, rnt_buf* key_b);
/* Gadget key-switch sum (engine.rs:505-528 / :429-452): for every poly of d
 * (coefficient domain): acc0 = sum_i alpha_i(d) * key_b[i],
 * acc1 = sum_i alpha_i(d) * key_a[i]; outputs coefficient domain. */
int rnt_keyswitch(rnt_buf* acc0, rnt_buf* acc1, const rnt_buf* d,
                  const rnt_buf* key_a, const rnt_buf* key_b);
/* mul_ciphertexts_gadget (engine.rs:473-539) for a batch of ciphertext
 * pairs: tensor product + gadget relinearization.  Inputs coefficient
 * domain; outputs coefficient domain. */
int rnt_ct_mul_relin(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0,
                     const rnt_buf* c1, const rnt_buf* c0p, const rnt_buf* c1p,
                     const rnt_buf* key_a, const rnt_buf* key_b);
/* mul_ciphertexts_gadget followed by rescale_ciphertext (engine.rs:473-539,
 * then :263-282), the engine's ct-mul call pair, as one op: out0/out1 are on
 * drop_last(1) of the inputs' basis (one shared context, as rnt_ct_rescale);
 * the result equals rnt_ct_mul_relin + rnt_ct_rescale word for word.  The
 * rescale runs as the key-switch inverse's epilogue, so the un-rescaled
 * product never reaches memory (N >= 2^14 with the four-step key-switch;
 * smaller rings run the two ops). */
int rnt_ct_mul_relin_rescale(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0,
                             const rnt_buf* c1, const rnt_buf* c0p, const rnt_buf* c1p,
                             const rnt_buf* key_a, const rnt_buf* key_b);
/* rotate_ciphertext (engine.rs:412-463). */
int rnt_ct_rotate(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0,
                  const rnt_buf* c1, int32_t k, const rnt_buf* key_a,
                  const rnt_buf* key_b);
/* The diagonal-method linear transform: for every ciphertext of the batch,
 *   out = sum_t diag[t] * rotate_ciphertext((c0, c1), steps[t]; key t),
 * word for word the composition rnt_ct_rotate -> coefficient-domain product
 * with diag[t] -> rnt_add.  c0, c1: coefficient domain; out0/out1 coefficient
 * domain on return (out0 == c0 and out1 == c1 allowed; any other aliasing of
 * an output -> RNT_ERR_BAD_ARGUMENT).  diag: n_terms polys, NTT domain (an
 * rnt_ntt_fwd result); poly t multiplies every ciphertext.  keys_a/keys_b:
 * n_terms * L prepared polys, term t's gadget key at [t L, (t + 1) L).  A term
 * with steps[t] == 0 is diag[t] * (c0, c1) without a key-switch (its key slot
 * is ignored; the key buffers may be NULL when every step is 0).  Where the
 * four-step key-switch runs the terms share its accumulators: one pair of
 * inverse column passes per chunk, the plaintext applied in the NTT domain. */
int rnt_ct_linear(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                  const int32_t* steps, size_t n_terms, const rnt_buf* diag,
                  const rnt_buf* keys_a, const rnt_buf* keys_b);
/* The same sum regrouped by baby steps and giant steps (a matrix whose
 * diagonal indices are giant_steps[j] + baby_steps[i]): for every ciphertext,
 *   R_i = rotate_ciphertext((c0, c1), baby_steps[i]; baby key i),
 *   V_j = sum_i diag[j n_baby + i] * R_i,
 *   out = sum_j rotate_ciphertext(V_j, giant_steps[j]; giant key j),
 * word for word that composition of rnt_ct_rotate, coefficient-domain products
 * and rnt_add: n_baby + n_giant key-switches at the most where rnt_ct_linear
 * runs one per diagonal.  A step of 0 in either list is the identity (its key
 * slot is ignored; a stage's key buffers may be NULL when all its steps are
 * 0); steps may be negative or repeated.  diag: n_giant * n_baby polys, NTT
 * domain, poly j n_baby + i multiplying every ciphertext of the batch.
 * baby_keys_a/b: n_baby * L prepared polys, giant_keys_a/b: n_giant * L, each
 * laid out as rnt_ct_linear's key set.  Domains and aliasing as rnt_ct_linear.
 * With n_giant == 1 and giant_steps[0] == 0 the result is rnt_ct_linear's on
 * steps = baby_steps.  (Not rnt_ct_linear's words on the same matrix: the
 * key-switch digits, and so the noise, differ.) */
int rnt_ct_linear_bsgs(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                       const int32_t* baby_steps, size_t n_baby,
                       const int32_t* giant_steps, size_t n_giant, const rnt_buf* diag,
                       const rnt_buf* baby_keys_a, const rnt_buf* baby_keys_b,
                       const rnt_buf* giant_keys_a, const rnt_buf* giant_keys_b);
/* ---- hoisted rotations: one gadget decomposition for many steps --------
 * For one ciphertext (c0, c1), a step k with sigma_k = rotate_slots(., k)
 * (poly.rs:546-569; for k < 0 its two-automorphism composition), that step's
 * ordinary gadget rotation key (key_a[i], key_b[i]) and the gadget digits
 * D_i = alpha_i(c1) (channel j of D_i = channel i of c1 mod q_j,
 * engine.rs:429-443), the hoisted rotation is
 *   out0 = sigma_k(c0) + sum_i sigma_k(D_i) * key_b[i]
 *   out1 =               sum_i sigma_k(D_i) * key_a[i]
 * (negacyclic products, coefficient domain, exact mod q_j, canonical outputs).
 * It is a valid rotation -- sum_i sigma(D_i) g_i = sigma(c1) mod Q, and sigma
 * only permutes and negates the digits, so the noise is rnt_ct_rotate's -- but
 * NOT rnt_ct_rotate's words, whose digits are alpha_i(sigma(c1)).  Because
 * sigma is a ring automorphism the same words are
 *   out0 = sigma_k(c0 + sum_i D_i * sigma_k^-1(key_b[i]))
 *   out1 = sigma_k(     sum_i D_i * sigma_k^-1(key_a[i]))
 * which is what runs: the transformed digits carry no step and are computed
 * once for every step; the step lives in the key's HOISTING FORM
 * NTT(sigma_k^-1(key)) and in one automorphism of the two sums.
 *
 * rnt_key_prepare_hoisted: (key_a, key_b) <- NTT(sigma_k^-1(key)), the hoisting
 * form of the gadget rotation key for step k.  Either domain on entry, NTT
 * domain on return; k == 0 is rnt_key_prepare.  A caller that needs both forms
 * of a key keeps two copies. */
int rnt_key_prepare_hoisted(rnt_buf* key_a, rnt_buf* key_b, int32_t k);
/* n_steps hoisted rotations (the definition above) of every ciphertext of the
 * batch with one decomposition.  c0, c1: B polys, coefficient domain (an
 * NTT-domain input -> RNT_ERR_DOMAIN_MISMATCH).  out0/out1: n_steps * B polys
 * on the same basis, rotation t of ciphertext b at poly t B + b, coefficient
 * domain on return.  A step of 0 is the identity (c0, c1) itself with no key;
 * steps may be negative or repeated.  keys_a/keys_b: n_steps * L polys laid out
 * as rnt_ct_linear's key set, step t's key in the hoisting form for steps[t]
 * (rnt_key_prepare_hoisted); a step-0 slot is ignored and the buffers may be
 * NULL when every step is 0; a coefficient-domain key ->
 * RNT_ERR_DOMAIN_MISMATCH, a wrong poly count -> RNT_ERR_CHANNEL_COUNT (fields:
 * expected, got).  n_steps == 0, outputs of the wrong size, an output aliasing
 * an input or the other output -> RNT_ERR_BAD_ARGUMENT.  The library cannot
 * tell an ordinary prepared key from a hoisting-form one: passing the wrong
 * form gives a wrong, not a rejected, result.  With a single step the call
 * pays the whole transform of the L^2 digits for it and is slower than
 * rnt_ct_rotate; it gains from the second step of the same ciphertext on. */
int rnt_ct_rotate_hoisted(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                          const int32_t* steps, size_t n_steps,
                          const rnt_buf* keys_a, const rnt_buf* keys_b);
/* rnt_ct_linear_bsgs with R_i defined by the hoisted rotation above instead of
 * rotate_ciphertext: every nonzero baby step shares one decomposition of c1.
 * baby_keys_a/b in hoisting form (rnt_key_prepare_hoisted with baby_steps[i]),
 * giant_keys_a/b ordinary (rnt_key_prepare).  Same argument rules otherwise.
 * Not rnt_ct_linear_bsgs' words: the baby digits differ. */
int rnt_ct_linear_bsgs_hoisted(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                               const int32_t* baby_steps, size_t n_baby,
                               const int32_t* giant_steps, size_t n_giant, const rnt_buf* diag,
                               const rnt_buf* baby_keys_a, const rnt_buf* baby_keys_b,
                               const rnt_buf* giant_keys_a, const rnt_buf* giant_keys_b);
/* ---- hybrid key-switching with special primes (DESIGN.md "Hybrid
 * key-switching") ---------------------------------------------------------
 * The ciphertext lives on a context C over q_0 .. q_{Lv-1}; the key on a
 * context E over q_0 .. q_{Lv-1}, p_0 .. p_{K-1} (K >= 1 special primes, P
 * their product).  E must have C's degree and device and its first Lv moduli
 * must equal C's BY VALUE: C may be E's drop_last(K) view, an unrelated root
 * or a view of another root, so a levelled ciphertext works with a per-level
 * key context.  The limbs are grouped into beta = ceil(Lv / alpha) digits of
 * alpha limbs (the last one may be partial), Q_d the product of digit d's.
 *   ModUp_d(x): y_i = x_i (Q_d/q_i)^-1 mod q_i for i in digit d; limb t of the
 *     result is x_t for t in the digit, else sum_i y_i (Q_d/q_i mod m_t) mod
 *     m_t (the fast base conversion: [x]_{Q_d} + u Q_d with 0 <= u < |digit|).
 *   A0 = sum_d ModUp_d(x) key_b[d], A1 with key_a (negacyclic, over E).
 *   ModDown(A): z_k = A_{p_k} (P/p_k)^-1 mod p_k; out_j = (A_j - sum_k z_k
 *     (P/p_k mod q_j)) P^-1 mod q_j (no rounding term: the floor-like
 *     quotient, off by at most K per coefficient).
 * rnt_keyswitch_hybrid: acc0 = ModDown(A0), acc1 = ModDown(A1) with x = d,
 * coefficient domain, canonical.  key_a / key_b: beta polys each over E,
 * prepared with rnt_key_prepare; the key for a target s' under s is
 * b_d = -a_d s + e_d + G_d with limb t of G_d = P s' mod q_t for t in digit d
 * and 0 elsewhere (all special limbs 0); the caller chooses P >~ alpha max Q_d.
 * At a lower level Lv' the key is the first ceil(Lv'/alpha) polys of the full
 * one restricted to the limbs q_0 .. q_{Lv'-1}, p_0 .. p_{K-1}, on a root
 * context over exactly those moduli -- or, without a copy, a key level view of
 * the full key (rnt_key_level_view, below).
 * Errors: alpha == 0, acc0 aliasing acc1 or d, batch sizes that differ ->
 * RNT_ERR_BAD_ARGUMENT; degree, device or moduli-prefix mismatch, or E without
 * a limb above C's -> RNT_ERR_BASIS_MISMATCH; E and C of different device word
 * widths -> RNT_ERR_UNSUPPORTED (fields 0, 0); a key poly count other than
 * beta -> RNT_ERR_CHANNEL_COUNT (fields: beta, got); a coefficient-domain key
 * or an NTT-domain d -> RNT_ERR_DOMAIN_MISMATCH.  The constants of (E, Lv,
 * alpha) are built on the first call, which therefore cannot be recorded
 * (rnt_capture_begin: run the sequence once first).  Launches run on C's
 * stream, after whatever E's stream held at the call. */
int rnt_keyswitch_hybrid(rnt_buf* acc0, rnt_buf* acc1, const rnt_buf* d,
                         const rnt_buf* key_a, const rnt_buf* key_b, size_t alpha);
/* rotate_ciphertext with the hybrid key-switch: (sigma_k(c0) + acc0, acc1) for
 * x = sigma_k(c1); k == 0 copies the input and does not read the key.  c0, c1
 * coefficient domain; the outputs may be the inputs (out0 == out1 ->
 * RNT_ERR_BAD_ARGUMENT).  Not rnt_ct_rotate's words: it decrypts alike, with
 * less noise. */
int rnt_ct_rotate_hybrid(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                         int32_t k, const rnt_buf* key_a, const rnt_buf* key_b, size_t alpha);
/* mul_ciphertexts_gadget with the hybrid key-switch: the tensor d0, d1, d2 of
 * rnt_ct_mul_relin, then (d0 + acc0, d1 + acc1) for x = d2; coefficient domain
 * in and out, aliasing as rnt_ct_mul_relin. */
int rnt_ct_mul_relin_hybrid(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                            const rnt_buf* c0p, const rnt_buf* c1p,
                            const rnt_buf* key_a, const rnt_buf* key_b, size_t alpha);
/* ---- key level views: one full-level hybrid key at every level -------------
 * The level-Lv' key is a subset of the full key's planes, so it needs no copy:
 * rnt_key_level_view makes a NON-owning, READ-ONLY buffer over `key`'s storage
 * on level_ctx (rnt_ctx_hybrid_level of key's context).  key: m beta polys,
 * beta = ceil(L / alpha), prepared (NTT domain, ordinary or hoisting form);
 * m = 1 is a key, m > 1 a packed key set.  The view reports m beta' polys,
 * beta' = ceil(level / alpha); its logical poly g beta' + d on working limb t
 * is the stored plane (r(t) m beta + g beta + d) N with r(t) the limb map
 * above: a set's steps keep the full key's poly stride beta.
 * A view is accepted as the key argument(s) of the nine hybrid calls
 * (rnt_keyswitch_hybrid, rnt_ct_rotate_hybrid, rnt_ct_mul_relin_hybrid,
 * rnt_ct_rotate_hybrid_hoisted, rnt_ct_linear_bsgs_hybrid,
 * rnt_ct_mul_relin_rescale_hybrid, rnt_ct_linear_bsgs_hybrid_rescale,
 * rnt_ct_dot_relin_hybrid, rnt_ct_dot_relin_rescale_hybrid), of
 * rnt_ct_rotsum_hybrid (the key set of a rotate-and-sum) and of
 * rnt_ct_mul_relin_rescale_affine_hybrid, which shares the multiply's body, and of
 * rnt_ct_linear_bsgs_hybrid_dh and its _rescale form (both key sets), and the
 * call is then, word for word, the same call with the restricted key on a
 * root context over the view's moduli.  Both halves (and both sets of a BSGS
 * call) must be views on the SAME level-context handle; a view at level == L
 * behaves as the key itself.  In any other position of any call a view ->
 * RNT_ERR_UNSUPPORTED (fields 0, 0) and nothing is touched.  rnt_buf_n_polys
 * and rnt_buf_is_ntt work on a view; rnt_buf_free releases the handle alone.
 * LIFETIME: the parent buffer must outlive its views, and a view reads the
 * parent's current words -- re-preparing or overwriting the parent changes
 * what the view reads.
 * Errors: key not on the context level_ctx was made from ->
 * RNT_ERR_BASIS_MISMATCH; a coefficient-domain key -> RNT_ERR_DOMAIN_MISMATCH;
 * alpha == 0, a level_ctx that is no level context, a view of a view, a null
 * argument -> RNT_ERR_BAD_ARGUMENT; a poly count that is no multiple of beta
 * -> RNT_ERR_CHANNEL_COUNT (fields: beta, got).  The first hybrid call of a
 * (view, alpha) pair builds its constants and cannot be recorded. */
int rnt_key_level_view(const rnt_buf* key, const rnt_ctx* level_ctx, size_t alpha, rnt_buf** out);
/* ---- hoisted rotations and the baby-step giant-step transform on hybrid
 * keys (DESIGN.md "Hoisted hybrid rotations") ------------------------------
 * Notation as above: C, E, beta = ceil(Lv / alpha), ModUp_d, ModDown; sigma_k =
 * rotate_slots(., k), one automorphism by g = 5^|k| (times 2N - 1 for k < 0).
 * The HOISTING FORM of a hybrid rotation key for step k is NTT(sigma_k^-1(a_d)),
 * NTT(sigma_k^-1(b_d)) over E for d < beta: rnt_key_prepare_hoisted(key_a,
 * key_b, k) on the beta-poly buffers over E (it works limb by limb, so the
 * restriction of a hoisting-form key to a lower level is the hoisting form of
 * the restricted key).  The hoisted hybrid rotation of (c0, c1) by k != 0, with
 * D_d = ModUp_d(c1) over E:
 *   out0 = sigma_k(c0 + ModDown(sum_d D_d * sigma_k^-1(key_b[d])))
 *   out1 = sigma_k(     ModDown(sum_d D_d * sigma_k^-1(key_a[d])))
 * (negacyclic products over E; canonical outputs, coefficient domain, over C);
 * k == 0 is the identity and does not read the key.  The ORDER is part of the
 * definition: ModDown is coefficient-wise but does not commute with negation
 * (on a negated coefficient the quotient differs by up to K), so sigma_k stands
 * outside ModDown.  It is also what runs: NTT(D_d) carries no step and is
 * computed once for every step.  It is a valid rotation -- sigma_k^-1(key)
 * switches from s to sigma_k^-1(s), the inner pair decrypts c0 + c1 s under
 * sigma_k^-1(s) and sigma_k of it the rotated message under s, with
 * rnt_ct_rotate_hybrid's error bound since sigma preserves norms -- but NOT
 * rnt_ct_rotate_hybrid's words: there ModUp sees sigma_k(c1).
 *
 * rnt_ct_rotate_hybrid_hoisted: n_steps such rotations of every ciphertext of
 * the batch with one ModUp and one forward transform.  c0, c1: B polys over C,
 * coefficient domain.  out0/out1: n_steps * B polys over C, rotation t of
 * ciphertext b at poly t B + b; no output aliases an input or the other output.
 * keys_a/keys_b: n_steps * beta polys over E, step t's key at [t beta, (t + 1)
 * beta) in the hoisting form for steps[t]; a step-0 slot is ignored and the
 * buffers may be NULL when every step is 0; steps may be negative or repeated.
 * Errors: rnt_keyswitch_hybrid's rules and statuses for alpha, degree, device,
 * moduli prefix, word width and key domain; a key set of another size ->
 * RNT_ERR_CHANNEL_COUNT (fields: n_steps * beta, got); n_steps == 0, outputs of
 * the wrong size, aliasing -> RNT_ERR_BAD_ARGUMENT; an NTT-domain ciphertext ->
 * RNT_ERR_DOMAIN_MISMATCH; a workspace that does not fit the device ->
 * RNT_ERR_OUT_OF_MEMORY.  A refused call leaves its outputs untouched.  The
 * library cannot tell a hoisting-form key from an ordinary one: passing the
 * wrong form gives a wrong, not a rejected, result.  The first call of an (E,
 * Lv, alpha) triple builds the constants and cannot be recorded. */
int rnt_ct_rotate_hybrid_hoisted(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                                 const int32_t* steps, size_t n_steps,
                                 const rnt_buf* keys_a, const rnt_buf* keys_b, size_t alpha);
/* The baby-step giant-step linear transform on hybrid keys.  diag[j n_baby + i]
 * in the NTT domain over C as rnt_ct_linear_bsgs takes it; baby keys in
 * hoisting form, giant keys ordinary (rnt_key_prepare), every key on one E with
 * one alpha, each set laid out as above (n beta polys).
 *   R_i = the hoisted hybrid rotation of (c0, c1) by b_i (the ciphertext itself
 *         for b_i = 0)
 *   V_j = sum_i diag[j n_baby + i] * R_i            (both components, over C)
 *   Z = { j : g_j = 0 }, NZ = the others
 *   A0 = sum_{j in NZ} sum_d ModUp_d(sigma_{g_j}(V1_j)) * giant_key_b[j][d]
 *        (over E); A1 with giant_key_a
 *   out0 = sum_{j in Z} V0_j + sum_{j in NZ} sigma_{g_j}(V0_j) + ModDown(A0)
 *   out1 = sum_{j in Z} V1_j                                  + ModDown(A1)
 * One ModDown per output component however many giants there are (none when NZ
 * is empty): NOT the words of a composition of rnt_ct_rotate_hybrid and rnt_add
 * -- a ModDown of a sum is not the sum of ModDowns -- but the same decryption,
 * the ModDown error entering once instead of |NZ| times.  With n_giant = 1 and
 * g_0 = 0 it is the diagonal-method transform over hoisted hybrid rotations.
 * Aliasing as rnt_ct_linear_bsgs (out0 == c0 and out1 == c1 allowed); a stage's
 * key buffers may be NULL when all its steps are 0; errors as above, and as
 * rnt_ct_linear_bsgs for the plaintexts; baby and giant keys on different key
 * bases -> RNT_ERR_BASIS_MISMATCH.  The library cannot tell a hoisting-form
 * key from an ordinary one. */
int rnt_ct_linear_bsgs_hybrid(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                              const int32_t* baby_steps, size_t n_baby,
                              const int32_t* giant_steps, size_t n_giant, const rnt_buf* diag,
                              const rnt_buf* baby_keys_a, const rnt_buf* baby_keys_b,
                              const rnt_buf* giant_keys_a, const rnt_buf* giant_keys_b, size_t alpha);
/* ---- rotate-and-sum on hybrid keys: one ModDown for many rotations
 * (DESIGN.md "Rotate-and-sum") ------------------------------------------------
 * The inner sum sum_t sigma_{k_t}(ct) of one stage of a slot sum.  Notation as
 * above: C, E, beta, ModUp_d, ModDown, sigma_k.  With NZ = {t : steps[t] != 0},
 * z = n_steps - |NZ| and D_d = ModUp_d(c1) over E:
 *   A0   = sum_{t in NZ} sum_d sigma_{k_t}(D_d) * key_b[t][d]   (negacyclic, over
 *          E);  A1 with key_a
 *   out0 = z c0 + sum_{t in NZ} sigma_{k_t}(c0) + ModDown(A0)
 *   out1 = z c1 +                                ModDown(A1)
 * Canonical outputs, coefficient domain, over C; z x is x added z times mod
 * q_j.  The keys are in the ORDINARY prepared form (rnt_key_prepare): the keys
 * rnt_ct_rotate_hybrid takes for step k_t, packed as the giant keys of
 * rnt_ct_linear_bsgs_hybrid are (n_steps * beta polys over E, step t's key at
 * [t beta, (t + 1) beta); a step-0 slot is ignored).  With NZ empty the result
 * is z ct, no key is read and the key buffers may be NULL.
 * The ORDER is part of the definition: sigma stands OUTSIDE ModUp and INSIDE
 * ModDown.  These are therefore NOT the words of a loop of rnt_ct_rotate_hybrid
 * and rnt_add -- ModUp does not commute with negation, and a ModDown of a sum
 * is not the sum of ModDowns -- but it decrypts the same way: sigma_k(D_d) ==
 * sigma_k(c1) mod Q_d with coefficients below alpha Q_d in magnitude (sigma
 * permutes coefficients up to sign), which is all the key-switch error bound
 * of rnt_ct_rotate_hybrid asks of ModUp_d(sigma_k(c1)); so every term has that
 * call's bound, and the ModDown error enters once instead of |NZ| times.
 * It is also what runs: one ModUp and one forward transform of the digits for
 * every step (in the NTT domain sigma_k is a gather, rnt_automorphism_ntt's),
 * |NZ| key streams into ONE accumulator pair, two inverse transforms over E and
 * two ModDowns, whatever n_steps is.  It spends no level and needs no plaintext.
 * c0, c1, out0, out1: B polys each on C, coefficient domain.  out0 == c0 and
 * out1 == c1 are allowed (a chain of stages runs in place); out0 == out1, an
 * output that is the other component or aliases a key -> RNT_ERR_BAD_ARGUMENT.
 * Every other rule and status is rnt_ct_rotate_hybrid_hoisted's: alpha, degree,
 * device, moduli prefix, word width, key domain, RNT_ERR_CHANNEL_COUNT (fields:
 * n_steps * beta, got), n_steps == 0 -> RNT_ERR_BAD_ARGUMENT, an NTT-domain
 * ciphertext -> RNT_ERR_DOMAIN_MISMATCH.  A refused call leaves its outputs
 * untouched.  Key level views are accepted in the key positions.  The library
 * cannot tell a hoisting-form key from an ordinary one.  The first call of an
 * (E, Lv, alpha) triple builds the constants and cannot be recorded; later
 * calls are recordable.  Profile names: "rotsum_mac" (the key products, 8 steps
 * a launch), "rotsum_c0" (the coefficient-domain sums). */
int rnt_ct_rotsum_hybrid(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                         const int32_t* steps, size_t n_steps,
                         const rnt_buf* keys_a, const rnt_buf* keys_b, size_t alpha);
/* polys [src_first, src_first + count) of src -> [dst_first, ...) of dst (same
 * context; dst takes src's domain, which must equal dst's unless the copy
 * covers all of dst).  A range outside either batch -> RNT_ERR_BAD_ARGUMENT. */
int rnt_copy_polys(rnt_buf* dst, size_t dst_first, const rnt_buf* src, size_t src_first,
                   size_t count);
/* rescale_ciphertext (engine.rs:263-282): both components onto the same
 * dropped basis. */
int rnt_ct_rescale(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0,
                   const rnt_buf* c1);
/* ---- the hybrid calls that close a level (DESIGN.md "Hybrid multiply and
 * linear transform with the rescale") ---------------------------------------
 * rnt_ct_mul_relin_rescale_hybrid is DEFINED as rnt_ct_mul_relin_hybrid
 * followed by rnt_ct_rescale, word for word: with r = ModDown(A) + d the level-Lv
 * result of the former (last limb r_last),
 *   out_j = (r_j - [r_last]_{q_j}) (q_last mod q_j)^-1 mod q_j,  j < Lv - 1,
 * canonical, coefficient domain.  r is never written: the seeds d0, d1 enter the
 * key products in the NTT domain (ModDown(A + P d) = ModDown(A) + d exactly,
 * since P d vanishes on the special limbs) and one kernel does ModDown and the
 * rescale.  c0, c1, c0p, c1p: B polys over C (Lv limbs), coefficient domain;
 * out0, out1: B polys on ONE shared context that is drop_last(1) of C, so no
 * output can be an input.
 * Errors: out0 == out1 -> RNT_ERR_BAD_ARGUMENT; inputs on different contexts
 * -> RNT_ERR_BASIS_MISMATCH, of different batch sizes -> RNT_ERR_BAD_ARGUMENT;
 * rnt_keyswitch_hybrid's rules and statuses for alpha (0 -> RNT_ERR_BAD_ARGUMENT),
 * degree, device, moduli prefix, word width, the key's poly count
 * (RNT_ERR_CHANNEL_COUNT, fields: beta, got) and a coefficient-domain key
 * (RNT_ERR_DOMAIN_MISMATCH); an NTT-domain input -> RNT_ERR_DOMAIN_MISMATCH;
 * then rnt_ct_mul_relin_rescale's output rules: a one-limb ciphertext ->
 * RNT_ERR_INVALID_MOD_DROP (fields: 1, Lv); an output whose context is not
 * drop_last(1) of C, or outputs on two contexts -> RNT_ERR_BASIS_MISMATCH; an
 * output of another batch size -> RNT_ERR_BAD_ARGUMENT.  A refused call leaves
 * its outputs untouched.  Recordable after one plain run of the (E, Lv, alpha)
 * triple, like the other hybrid calls. */
int rnt_ct_mul_relin_rescale_hybrid(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                                    const rnt_buf* c0p, const rnt_buf* c1p,
                                    const rnt_buf* key_a, const rnt_buf* key_b, size_t alpha);
/* The fused multiply-add on a hybrid key (DESIGN.md "Fused multiply-add and
 * EvalMod").  With (r0, r1) the result of rnt_ct_mul_relin_rescale_hybrid on
 * the same inputs,
 *   out0 = w r0 + u z0 + bias X^0      out1 = w r1 + u z1
 * exactly mod every q_t, canonical, coefficient domain: DEFINED as that call
 * followed by rnt_ct_lincomb on [r, z] with weights (w, u) and bias `bias`,
 * word for word.  The affine step is the epilogue of the two kernels that
 * close the multiply (profile name "moddown_rescale_affine"): the launch count
 * is the plain call's, r is never written and w, u, bias travel by value -- no
 * host array is copied, so unlike rnt_ct_lincomb the call can be recorded.
 * z0, z1: both NULL (u is ignored) or both given, B polys on the outputs'
 * context, coefficient domain; z0 == out0 together with z1 == out1 is allowed
 * (accumulation in place).  w, u, bias are signed integers, reduced mod q_t
 * by the kernel (a negative one as q_t - |.| mod q_t).
 * Errors: every rule and status of rnt_ct_mul_relin_rescale_hybrid (key level
 * views in the key positions included), then |w| >= 2^31, |bias| >= 2^62, an
 * output that aliases an input, only one of z0 / z1 given, |u| >= 2^31 (with
 * addends), an addend of another batch size, an addend that overlaps an
 * output other than z0 == out0 with z1 == out1 -> RNT_ERR_BAD_ARGUMENT; an
 * addend that is a key level view -> RNT_ERR_UNSUPPORTED; on another context
 * than the outputs' -> RNT_ERR_BASIS_MISMATCH; in the NTT domain ->
 * RNT_ERR_DOMAIN_MISMATCH.  A refused call leaves its outputs untouched.
 * Recordable after one plain run of the (E, Lv, alpha) triple. */
int rnt_ct_mul_relin_rescale_affine_hybrid(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                                           const rnt_buf* c0p, const rnt_buf* c1p,
                                           const rnt_buf* key_a, const rnt_buf* key_b, size_t alpha,
                                           int64_t w, const rnt_buf* z0, const rnt_buf* z1, int64_t u,
                                           int64_t bias);
/* rnt_ct_linear_bsgs_hybrid followed by rnt_ct_rescale, word for word: the same
 * arguments, the outputs as above (B polys on one shared drop_last(1) of C, so
 * none aliases an input).  With a nonzero giant step the two closing ModDowns
 * and the rescale are one kernel each; with none (the diagonal method) there is
 * no ModDown and the rescale kernel reads the sums.  Errors: those of
 * rnt_ct_linear_bsgs_hybrid for steps, plaintexts, keys, alpha and domains, then
 * the output rules above with their statuses and fields. */
int rnt_ct_linear_bsgs_hybrid_rescale(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                                      const int32_t* baby_steps, size_t n_baby,
                                      const int32_t* giant_steps, size_t n_giant, const rnt_buf* diag,
                                      const rnt_buf* baby_keys_a, const rnt_buf* baby_keys_b,
                                      const rnt_buf* giant_keys_a, const rnt_buf* giant_keys_b, size_t alpha);
/* ---- the double-hoisted baby-step giant-step transform on hybrid keys
 * (DESIGN.md "Double-hoisted hybrid BSGS"; Bossuat et al. 2021) ---------------
 * rnt_ct_linear_bsgs_hybrid with the baby rotations never taken down from
 * Q u P.  Notation and key sets as that call's: C, E, P = prod p_k, beta,
 * ModUp_d, ModDown, sigma_k; baby keys in the HOISTING form, giant keys
 * ordinary, so one pair of key sets serves both calls.  diagE[j n_baby + i] is
 * the encoded integer polynomial of that call's diag reduced mod every modulus
 * of E, in the NTT domain, on a context whose moduli equal q_0..q_{Lv-1},
 * p_0..p_{K-1} BY VALUE (the keys' root E, or any context over those moduli).
 * With D_d = ModUp_d(c1), all products negacyclic over E:
 *   b_i != 0: T0_i = P c0 + sum_d D_d sigma_{b_i}^-1(key_b[i][d])   (P c0: [P]_{q_j} c0
 *             T1_i =        sum_d D_d sigma_{b_i}^-1(key_a[i][d])    on q_j, 0 on p_k)
 *             Rt_i = (sigma_{b_i}(T0_i), sigma_{b_i}(T1_i))   over E: no ModDown, sigma exact
 *   b_i == 0: Rt_i = (P c0, P c1)                             over E, no key read
 *   Vt_j = sum_i diagE[j n_baby + i] Rt_i                     both components, over E
 *   Z = { j : g_j = 0 }, NZ = the others;  W_j = ModDown(Vt1_j) over C for j in NZ
 *   A0 = sum_{j in Z} Vt0_j + sum_{j in NZ} (sigma_{g_j}(Vt0_j)
 *                                + sum_d ModUp_d(sigma_{g_j}(W_j)) giant_key_b[j][d])
 *   A1 = sum_{j in Z} Vt1_j + sum_{j in NZ} sum_d ModUp_d(sigma_{g_j}(W_j)) giant_key_a[j][d]
 *   out0 = ModDown(A0), out1 = ModDown(A1)      canonical, coefficient domain, over C
 * There is no special case: with every step 0 the result is ModDown(P x) = x,
 * the call equals sum diag c word for word and no key buffer is read (they may
 * be NULL; E is then the plaintexts' context).  NOT the words of
 * rnt_ct_linear_bsgs_hybrid -- the ModDowns are grouped differently -- but the
 * same decryption; the baby ModDown roundings are no longer multiplied by the
 * plaintexts.  ModDowns per chunk: |NZ| + 2 instead of 2 nz_baby + 2; the price
 * is inner sums and plaintexts over Lv + K limbs instead of Lv.
 * rnt_ct_linear_bsgs_hybrid_dh_rescale is that result followed by
 * rnt_ct_rescale, word for word (outputs as rnt_ct_linear_bsgs_hybrid_rescale's).
 * Rules and statuses are rnt_ct_linear_bsgs_hybrid's (aliasing: out0 == c0 and
 * out1 == c1 allowed; key level views in the key positions; a stage's key
 * buffers NULL when all its steps are 0), with these for the plaintexts: a
 * context whose moduli are not E's at this level by value, or of another degree
 * or device -> RNT_ERR_BASIS_MISMATCH; another word width -> RNT_ERR_UNSUPPORTED;
 * a poly count other than n_baby n_giant -> RNT_ERR_CHANNEL_COUNT (fields:
 * n_baby n_giant, got); coefficient domain -> RNT_ERR_DOMAIN_MISMATCH; an
 * output that shares its storage with the plaintexts, a key set or the other
 * component's input (a wrapped buffer included) -> RNT_ERR_BAD_ARGUMENT.  A
 * refused call leaves its outputs untouched.  ORDER: the call runs on the
 * ciphertext context's stream; where the plaintexts live on another root
 * context (its own stream), the call first orders itself after everything
 * queued on that stream so far, as it does for the key basis and as
 * rnt_mod_raise does for its input, so plaintexts uploaded or transformed just
 * before the call need no rnt_sync.  (Not inside a capture: a recorded call
 * reads plaintexts that are ready.)  The first call of an (E, Lv,
 * alpha) triple builds the constants and cannot be recorded; later calls are
 * recordable.  Profile names: "dh_bsgs_mac" (the inner sums over E, 4 giants
 * and 16 babies a launch), "dh_bsgs_fold" (the first components into A0 / A1,
 * 4 giants a launch). */
int rnt_ct_linear_bsgs_hybrid_dh(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                                 const int32_t* baby_steps, size_t n_baby,
                                 const int32_t* giant_steps, size_t n_giant, const rnt_buf* diagE,
                                 const rnt_buf* baby_keys_a, const rnt_buf* baby_keys_b,
                                 const rnt_buf* giant_keys_a, const rnt_buf* giant_keys_b, size_t alpha);
int rnt_ct_linear_bsgs_hybrid_dh_rescale(rnt_buf* out0, rnt_buf* out1, const rnt_buf* c0, const rnt_buf* c1,
                                         const int32_t* baby_steps, size_t n_baby,
                                         const int32_t* giant_steps, size_t n_giant, const rnt_buf* diagE,
                                         const rnt_buf* baby_keys_a, const rnt_buf* baby_keys_b,
                                         const rnt_buf* giant_keys_a, const rnt_buf* giant_keys_b, size_t alpha);
/* ---- scalar linear combinations of ciphertexts (DESIGN.md "Scalar linear
 * combinations and polynomial evaluation") --------------------------------
 * The scalar path of a circuit: ciphertext x constant, ciphertext + constant
 * and every weighted sum of a set of ciphertexts, n_out of them from n_in
 * inputs in one launch.  x0, x1: n_in B polys over a context C with Lv limbs,
 * coefficient domain, term i of ciphertext b at poly i B + b (the layout
 * rnt_ct_rotate_hybrid_hoisted writes).  weights: host uint64_t[n_out][n_in][Lv],
 * residues mod q_t; bias: host uint64_t[n_out][Lv] or NULL for none.  For
 * output j, ciphertext b, limb t, exact mod q_t and canonical:
 *   r0 = sum_i w[j][i][t] x0_i + bias[j][t] X^0
 *   r1 = sum_i w[j][i][t] x1_i
 * (the bias on coefficient 0 of component 0 alone: a constant polynomial is
 * that constant in every slot).  rnt_ct_lincomb writes (r0, r1): out0 / out1
 * hold n_out B polys over C, output j of ciphertext b at poly j B + b,
 * coefficient domain.  No output aliases an input or the other output.
 * Errors: n_in or n_out of 0, inputs whose poly counts differ or are no
 * multiple of n_in, outputs of other than n_out B polys, aliasing, null
 * weights -> RNT_ERR_BAD_ARGUMENT; n_in or n_out above 16 -> RNT_ERR_UNSUPPORTED
 * (fields 0, 0); a weight or bias >= its modulus -> RNT_ERR_NON_REDUCED
 * (fields: value, modulus); an NTT-domain input -> RNT_ERR_DOMAIN_MISMATCH;
 * inputs on different contexts, or an output on another context than the
 * inputs' -> RNT_ERR_BASIS_MISMATCH; a key level view in any position ->
 * RNT_ERR_UNSUPPORTED.  A refused call leaves its outputs untouched.
 * Both host arrays are read during the call (packed into staging memory the
 * library owns and copied up on the context's stream); the caller may free
 * them on return.  That host copy is one a graph cannot own, so the call CANNOT
 * be recorded: between rnt_capture_begin and rnt_capture_end it returns
 * RNT_ERR_UNSUPPORTED (fields 0, 0) and records nothing. */
int rnt_ct_lincomb(rnt_buf* out0, rnt_buf* out1, const rnt_buf* x0, const rnt_buf* x1,
                   size_t n_in, size_t n_out, const uint64_t* weights, const uint64_t* bias);
/* rnt_ct_lincomb followed by rnt_ct_rescale, word for word: the outputs are
 * n_out B polys on ONE shared context that is drop_last(1) of C,
 *   out_t = (r_t - [r_last]_{q_t}) (q_last mod q_t)^-1 mod q_t,  t < Lv - 1,
 * and r is never written to memory.  Errors as above, then
 * rnt_ct_mul_relin_rescale's output rules: Lv == 1 -> RNT_ERR_INVALID_MOD_DROP
 * (fields: 1, Lv); an output whose context is not drop_last(1) of C, or outputs
 * on two contexts -> RNT_ERR_BASIS_MISMATCH.  Not recordable, as above. */
int rnt_ct_lincomb_rescale(rnt_buf* out0, rnt_buf* out1, const rnt_buf* x0, const rnt_buf* x1,
                           size_t n_in, size_t n_out, const uint64_t* weights, const uint64_t* bias);
/* ---- ciphertext inner products with one relinearisation (DESIGN.md "Hybrid
 * inner product with a single relinearisation") ------------------------------
 * A sum of n_terms ciphertext x ciphertext products whose three tensor
 * components are summed BEFORE the key-switch (lazy relinearisation).  x0, x1,
 * y0, y1: n_terms B polys over a context C with Lv limbs, coefficient domain,
 * term i of ciphertext b at poly i B + b (the layout rnt_ct_lincomb reads and
 * rnt_ct_rotate_hybrid_hoisted writes).  With negacyclic products, exact mod
 * every q_t:
 *   d0 = sum_i x0_i y0_i   d1 = sum_i (x0_i y1_i + x1_i y0_i)   d2 = sum_i x1_i y1_i
 *   (acc0, acc1) = rnt_keyswitch_hybrid(d2; key_a, key_b, alpha)
 *   out = (d0 + acc0, d1 + acc1)        B polys over C, canonical, coefficient domain.
 * These ARE the words of the composition "coefficient-domain rnt_mul and
 * rnt_add for d0, d1, d2, then rnt_keyswitch_hybrid and rnt_add", and with
 * n_terms == 1 the words of rnt_ct_mul_relin_hybrid.  With n_terms > 1 they
 * are NOT the words of the sum of n_terms rnt_ct_mul_relin_hybrid results -- a
 * ModDown of a sum is not the sum of ModDowns -- but the same decryption, the
 * key-switch error entering once instead of n_terms times.  Any n_terms >= 1
 * is valid: the terms are transformed and summed in groups, the key-switch
 * runs once a chunk of ciphertexts.
 * y may be x: y0 == x0 together with y1 == x1 is a sum of squares (each plane
 * is then transformed once).  The inputs are never written.  No output
 * aliases an input or the other output -> RNT_ERR_BAD_ARGUMENT.
 * Errors: n_terms == 0, input poly counts that differ or are no multiple of
 * n_terms, outputs of other than B polys -> RNT_ERR_BAD_ARGUMENT; inputs on
 * different contexts, or an output on another context than the inputs' ->
 * RNT_ERR_BASIS_MISMATCH; an NTT-domain input -> RNT_ERR_DOMAIN_MISMATCH;
 * rnt_keyswitch_hybrid's rules and statuses for alpha, degree, device, moduli
 * prefix, word width, the key's poly count (RNT_ERR_CHANNEL_COUNT, fields:
 * beta, got) and the key's domain.  A key level view is accepted in the key
 * positions, where it behaves word for word like the restricted key; in any
 * other position -> RNT_ERR_UNSUPPORTED.  A refused call leaves its outputs
 * untouched.  No host array is read: recordable after one plain run of the
 * (E, Lv, alpha) triple, like the other hybrid calls. */
int rnt_ct_dot_relin_hybrid(rnt_buf* out0, rnt_buf* out1, const rnt_buf* x0, const rnt_buf* x1,
                            const rnt_buf* y0, const rnt_buf* y1, size_t n_terms,
                            const rnt_buf* key_a, const rnt_buf* key_b, size_t alpha);
/* rnt_ct_dot_relin_hybrid followed by rnt_ct_rescale, word for word (with
 * n_terms == 1 the words of rnt_ct_mul_relin_rescale_hybrid): out0, out1 hold B
 * polys on ONE shared context that is drop_last(1) of C.  Errors as above,
 * then rnt_ct_mul_relin_rescale_hybrid's output rules: Lv == 1 ->
 * RNT_ERR_INVALID_MOD_DROP (fields: 1, Lv); an output whose context is not
 * drop_last(1) of C, or outputs on two contexts -> RNT_ERR_BASIS_MISMATCH; an
 * output of other than B polys -> RNT_ERR_BAD_ARGUMENT. */
int rnt_ct_dot_relin_rescale_hybrid(rnt_buf* out0, rnt_buf* out1, const rnt_buf* x0, const rnt_buf* x1,
                                    const rnt_buf* y0, const rnt_buf* y1, size_t n_terms,
                                    const rnt_buf* key_a, const rnt_buf* key_b, size_t alpha);

/* ---- ciphertext x plaintext multiply-accumulate (DESIGN.md "Plaintext
 * multiply-accumulate") ------------------------------------------------------
 * sum_i w_i (.) ct_i + b with encoded plaintext vectors w_i and b: a dense layer
 * over pre-rotated ciphertexts, a slot mask, per-slot coefficients.  No key is
 * involved.  Two calls: rnt_ct_plain_mac, and rnt_ct_plain_mac_rescale, which
 * closes the level as well.  x0, x1: n_terms B polys over a context C with Lv limbs,
 * coefficient domain, term i of ciphertext b at poly i B + b (the layout
 * rnt_ct_lincomb and rnt_ct_dot_relin_hybrid read and
 * rnt_ct_rotate_hybrid_hoisted writes).  m: the plaintexts in the NTT domain on
 * C (as the diag of rnt_ct_linear), either n_terms polys -- plaintext i shared
 * by every ciphertext of the batch -- or n_terms B polys, term i of ciphertext
 * b at poly i B + b.  bias: NULL, or 1 poly (shared) or B polys, NTT domain on
 * C.  With negacyclic products, exact mod every q_t and canonical:
 *   r0_b = sum_i x0_{i,b} m_{i(,b)} + bias_{(b)}      r1_b = sum_i x1_{i,b} m_{i(,b)}
 * rnt_ct_plain_mac writes (r0, r1): B polys over C, coefficient domain.  These
 * ARE the words of the coefficient-domain composition: rnt_mul of each term
 * with the plaintext taken back to coefficients (rnt_ntt_inv), rnt_add over the
 * terms and the bias.  Any n_terms >= 1 is valid: the terms are transformed and
 * summed in groups, a batch in chunks within RNT_KS_WS_MB of workspace; two
 * inverse transforms a chunk whatever n_terms is.  The plaintexts are read
 * where they lie; the inputs are never written.  No host array is read: both
 * calls can be recorded after one plain run.
 * Errors (a refused call leaves its outputs untouched):
 *   n_terms == 0                                           RNT_ERR_BAD_ARGUMENT
 *   x0 / x1 poly counts that differ or are no multiple
 *     of n_terms                                           RNT_ERR_BAD_ARGUMENT
 *   m of neither n_terms nor n_terms B polys               RNT_ERR_BAD_ARGUMENT
 *   bias of neither 1 nor B polys                          RNT_ERR_BAD_ARGUMENT
 *   outputs of other than B polys                          RNT_ERR_BAD_ARGUMENT
 *   an output that aliases an input or the other output    RNT_ERR_BAD_ARGUMENT
 *   inputs, plaintexts or bias on different contexts       RNT_ERR_BASIS_MISMATCH
 *   an un-rescaled output on another context than the
 *     inputs'                                              RNT_ERR_BASIS_MISMATCH
 *   an NTT-domain x0 / x1                                  RNT_ERR_DOMAIN_MISMATCH
 *   a coefficient-domain m or bias                         RNT_ERR_DOMAIN_MISMATCH
 *   a key level view in any position                       RNT_ERR_UNSUPPORTED (fields 0, 0)
 *   the rescaling call with Lv == 1                        RNT_ERR_INVALID_MOD_DROP (fields: 1, Lv)
 *   the rescaling call with outputs on the wrong or on
 *     two contexts                                         RNT_ERR_BASIS_MISMATCH */
int rnt_ct_plain_mac(rnt_buf* out0, rnt_buf* out1, const rnt_buf* x0, const rnt_buf* x1,
                     const rnt_buf* m, const rnt_buf* bias, size_t n_terms);
/* rnt_ct_plain_mac followed by rnt_ct_rescale, word for word: out0, out1 hold B
 * polys on ONE shared context that is drop_last(1) of C (the output rules of
 * rnt_ct_mul_relin_rescale_hybrid).  Errors as in the table above. */
int rnt_ct_plain_mac_rescale(rnt_buf* out0, rnt_buf* out1, const rnt_buf* x0, const rnt_buf* x1,
                             const rnt_buf* m, const rnt_buf* bias, size_t n_terms);

/* ---- limb-sharded building blocks ------------------------ */
/* A rank owning a contiguous run of the global basis' limbs holds every
 * ciphertext restricted to them (a context over those moduli).  The join
 * steps take the other ranks' limbs as raw device arrays gathered by the
 * caller. */
/* Tensor product of mul_ciphertexts_gadget (engine.rs:480-493) on the local
 * limbs: d0 = c0 c0', d1 = c0 c1' + c1 c0' (NTT domain, device order: the
 * seeds of rnt_keyswitch_ext), d2 = c1 c1' (coefficient domain). */
int rnt_ct_tensor(rnt_buf* d0, rnt_buf* d1, rnt_buf* d2, const rnt_buf* c0,
                  const rnt_buf* c1, const rnt_buf* c0p, const rnt_buf* c1p);
/* Gadget sum (engine.rs:505-528) for the local (target) limbs of acc0/acc1
 * over `src_limbs` source limbs held at `src` ([src_limbs][B][N] words,
 * coefficient domain, B = acc0's batch): acc = INV(seed + sum_i
 * NTT(src_i mod q_j) key[i]); key_a/key_b hold src_limbs polys over acc's
 * basis (prepared); init0/init1 NTT-domain seeds or NULL. */
int rnt_keyswitch_ext(rnt_buf* acc0, rnt_buf* acc1, const void* src, size_t src_limbs,
                      const rnt_buf* key_a, const rnt_buf* key_b, const rnt_buf* init0,
                      const rnt_buf* init1);
/* rescale_into (poly.rs:187-228) by an external last modulus q_last whose
 * residues (coefficient domain, [B][N] words) are at `last_limb`: every
 * local limb l -> (c_l - (c_last mod q_l)) (q_last mod q_l)^-1.  If q_last is
 * the input's own last modulus (the shard that owns it) that limb is
 * dropped, so `out` must be drop_last(1) of `in`'s context; otherwise `out`
 * shares `in`'s context. */
int rnt_rescale_ext(rnt_buf* out, const rnt_buf* in, const void* last_limb, uint64_t q_last);

#ifdef __cplusplus
}
#endif
#endif /* RNSNTT_H */
