// affine_args_check.cpp -- the argument rules of
// rnt_ct_mul_relin_rescale_affine_hybrid on the host alone, as a stand-alone
// program for a sanitizer build of rnt_api.cpp (tools/sanitize_affine_args.sh).
//
// Every refusal of the call is decided before any device work, from the
// handles' host fields only.  The program builds contexts and buffers by hand
// (rnt_internal.hpp: no table is allocated, the data pointers are never
// dereferenced and never reach a launch), sends every refused combination and
// compares the status.  It makes no valid call, so it needs no GPU.
#include <cinttypes>
#include <cstdio>
#include <memory>

#include "rnsntt.h"
#include "rnt_internal.hpp"

namespace {

int g_failed = 0;

void expect(const char* what, int got, int want) {
  if (got != want) {
    std::printf("FAIL %s: status %d (%s), expected %d\n", what, got, rnt_last_error(), want);
    ++g_failed;
  } else {
    std::printf("ok   %s: %d\n", what, got);
  }
}

// Tables that are never destroyed (their destructor frees device memory).
std::shared_ptr<rnt::Tables> tables(std::initializer_list<uint64_t> moduli) {
  auto* t = new rnt::Tables;
  t->log_n = 8;
  t->n = 256;
  t->moduli.assign(moduli);
  t->L = t->moduli.size();
  return std::shared_ptr<rnt::Tables>(t, [](rnt::Tables*) {});
}

rnt_ctx* context(const std::shared_ptr<rnt::Tables>& t, size_t L) {
  auto* c = new rnt_ctx;
  c->t = t;
  c->L = L;
  return c;
}

rnt_buf* buffer(const rnt_ctx* ctx, size_t n_polys, int in_ntt = 0) {
  static uintptr_t next = 0x10000;
  auto* b = new rnt_buf;
  b->ctx = ctx;
  b->n_polys = n_polys;
  b->data = reinterpret_cast<void*>(next);  // distinct, aligned, never dereferenced
  next += 0x10000;
  b->in_ntt = in_ntt;
  return b;
}

}  // namespace

int main() {
  const uint64_t q0 = 2147473409ull, q1 = 2147469313ull, q2 = 2147465729ull, p0 = 2147462143ull, p1 = 2147459329ull;
  const size_t B = 2, alpha = 2;
  auto tc = tables({q0, q1, q2, p0, p1});
  rnt_ctx* E = context(tc, 5);    // the key basis
  rnt_ctx* C = context(tc, 3);    // the ciphertexts': its drop_last(2)
  rnt_ctx* low = context(tc, 2);  // the outputs': drop_last(1) of C
  rnt_ctx* low2 = context(tc, 2); // the same limbs on a context of their own
  rnt_buf *o0 = buffer(low, B), *o1 = buffer(low, B);
  rnt_buf *c0 = buffer(C, B), *c1 = buffer(C, B), *c0p = buffer(C, B), *c1p = buffer(C, B);
  rnt_buf *ka = buffer(E, 2, 1), *kb = buffer(E, 2, 1);
  rnt_buf *z0 = buffer(low, B), *z1 = buffer(low, B);
  rnt_buf view = *z0;  // a key level view in an addend position
  view.view_of = ka;
  const int64_t W31 = (int64_t)1 << 31, B62 = (int64_t)1 << 62;

  auto call = [&](rnt_buf* out0, rnt_buf* out1, int64_t w, const rnt_buf* a0, const rnt_buf* a1, int64_t u,
                  int64_t bias) {
    return rnt_ct_mul_relin_rescale_affine_hybrid(out0, out1, c0, c1, c0p, c1p, ka, kb, alpha, w, a0, a1, u, bias);
  };
  expect("w = 2^31", call(o0, o1, W31, z0, z1, 1, 0), RNT_ERR_BAD_ARGUMENT);
  expect("w = -2^31", call(o0, o1, -W31, z0, z1, 1, 0), RNT_ERR_BAD_ARGUMENT);
  expect("w = INT64_MIN", call(o0, o1, INT64_MIN, z0, z1, 1, 0), RNT_ERR_BAD_ARGUMENT);
  expect("u = 2^31", call(o0, o1, 1, z0, z1, W31, 0), RNT_ERR_BAD_ARGUMENT);
  expect("u = INT64_MIN", call(o0, o1, 1, z0, z1, INT64_MIN, 0), RNT_ERR_BAD_ARGUMENT);
  expect("bias = 2^62", call(o0, o1, 1, z0, z1, 1, B62), RNT_ERR_BAD_ARGUMENT);
  expect("bias = -2^62", call(o0, o1, 1, z0, z1, 1, -B62), RNT_ERR_BAD_ARGUMENT);
  expect("bias = INT64_MIN", call(o0, o1, 1, nullptr, nullptr, 0, INT64_MIN), RNT_ERR_BAD_ARGUMENT);
  expect("z1 alone", call(o0, o1, 1, nullptr, z1, 1, 0), RNT_ERR_BAD_ARGUMENT);
  expect("z0 alone", call(o0, o1, 1, z0, nullptr, 1, 0), RNT_ERR_BAD_ARGUMENT);
  expect("z0 a key level view", call(o0, o1, 1, &view, z1, 1, 0), RNT_ERR_UNSUPPORTED);
  expect("z1 a key level view", call(o0, o1, 1, z0, &view, 1, 0), RNT_ERR_UNSUPPORTED);
  expect("z0 on another context", call(o0, o1, 1, buffer(low2, B), z1, 1, 0), RNT_ERR_BASIS_MISMATCH);
  expect("z1 on the inputs' context", call(o0, o1, 1, z0, buffer(C, B), 1, 0), RNT_ERR_BASIS_MISMATCH);
  expect("z0 of another batch", call(o0, o1, 1, buffer(low, B + 1), z1, 1, 0), RNT_ERR_BAD_ARGUMENT);
  expect("z1 in the NTT domain", call(o0, o1, 1, z0, buffer(low, B, 1), 1, 0), RNT_ERR_DOMAIN_MISMATCH);
  expect("z0 == out0 alone", call(o0, o1, 1, o0, z1, 1, 0), RNT_ERR_BAD_ARGUMENT);
  expect("z1 == out1 alone", call(o0, o1, 1, z0, o1, 1, 0), RNT_ERR_BAD_ARGUMENT);
  expect("addends crossed", call(o0, o1, 1, o1, o0, 1, 0), RNT_ERR_BAD_ARGUMENT);
  rnt_buf alias = *z0;  // another handle of out1's words
  alias.data = o1->data;
  expect("z0 on out1's words", call(o0, o1, 1, &alias, z1, 1, 0), RNT_ERR_BAD_ARGUMENT);
  rnt_buf in_alias = *o0;  // an output on an input's words
  in_alias.data = c1p->data;
  expect("out0 on c1p's words", call(&in_alias, o1, 1, z0, z1, 1, 0), RNT_ERR_BAD_ARGUMENT);
  // the multiply's own rules come first
  expect("out0 == out1", call(o0, o0, 1, z0, z1, 1, 0), RNT_ERR_BAD_ARGUMENT);
  expect("outputs on two contexts", call(o0, buffer(low2, B), 1, z0, z1, 1, 0), RNT_ERR_BASIS_MISMATCH);
  expect("an output at the inputs' level", call(buffer(C, B), o1, W31, z0, z1, 1, 0), RNT_ERR_BASIS_MISMATCH);
  expect("null output", call(nullptr, o1, 1, z0, z1, 1, 0), RNT_ERR_BAD_ARGUMENT);
  expect("alpha = 0",
         rnt_ct_mul_relin_rescale_affine_hybrid(o0, o1, c0, c1, c0p, c1p, ka, kb, 0, 1, z0, z1, 1, 0),
         RNT_ERR_BAD_ARGUMENT);
  std::printf("%s: %d failure(s)\n", g_failed ? "FAILED" : "PASSED", g_failed);
  return g_failed ? 1 : 0;
}
