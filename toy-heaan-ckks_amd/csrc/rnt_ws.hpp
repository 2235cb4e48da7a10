// rnt_ws.hpp -- the layout of a call-scoped workspace block: every part is
// declared once, in order, and the block's size, the parts' addresses and the
// planes a ciphertext of a chunk costs all come from those declarations.  A
// part is a fixed byte count, `count` chunk blocks of [limbs][bc][N] words, or
// a nested layout; a part of no bytes has the address nullptr.  Host only and
// free of the HIP headers (tests/cpp/test_ws_layout.cpp compiles it alone).
#pragma once
#include <algorithm>
#include <cassert>
#include <cstddef>

namespace rnt {

struct WsLayout {
  // A part: its fixed bytes; the planes per poly of one block, and the blocks; the fixed bytes and planes before it.
  struct Slot {
    size_t fixed, limbs, count, fixed0, planes0;
  };
  size_t n, wb;  // words per plane, bytes per word
  Slot slot[12];
  int slots = 0;
  size_t fixed = 0, planes = 0;  // fixed bytes; planes of N words per poly of a chunk
  size_t bc = 0;                 // polys the blocks are pitched for
  char* base = nullptr;

  WsLayout(size_t n_, size_t wb_) : n(n_), wb(wb_) {}
  WsLayout& add(size_t bytes, size_t limbs, size_t count) {
    assert(slots < 12 && !base);
    slot[slots++] = {bytes, limbs, count, fixed, planes};
    fixed += bytes;
    planes += limbs * count;
    return *this;
  }
  WsLayout& bytes(size_t b) { return add(b, 0, 0); }
  WsLayout& blocks(size_t limbs, size_t count = 1) { return add(0, limbs, count); }
  WsLayout& sub(const WsLayout& s) { return add(s.fixed, s.planes, 1); }
  WsLayout& chunk(size_t polys) {
    bc = polys;
    return *this;
  }
  // What CallWs::get is asked for (`floor`: the allocator's, where a call has one).
  size_t total(size_t floor = 0) const {
    assert(bc != 0 || planes == 0);
    return std::max(fixed + planes * bc * n * wb, floor);
  }
  WsLayout& place(void* p) {
    assert(p != nullptr || total() == 0);
    base = (char*)p;
    return *this;
  }
  size_t pitch(int i) const { return slot[i].limbs * bc * n * wb; }  // one block of part i
  // Block `block` of part i, within the total by construction; nullptr for a part of no bytes.
  char* at(int i, size_t block = 0) const {
    assert(i >= 0 && i < slots);
    const Slot& s = slot[i];
    if (s.fixed + s.limbs * s.count == 0) return nullptr;
    assert(base != nullptr && block < std::max<size_t>(s.count, 1));
    return base + s.fixed0 + (s.planes0 + block * s.limbs) * bc * n * wb;
  }
};

// The two scratch layouts every key-switch call nests, sized for the call's chunk (chunk(bc)) and carved per chunk
// at the chunk's own pitch (chunk(c).place(p)): a last, smaller chunk packs its parts closer.  Gadget: the
// decomposition S ([Lt][Ls][c][N]) | the NTT-row accumulators U0 | U1 ([Lt][c][N]); the whole-plane key-switch has
// none (and no part to ask for: nothing carves it there).
enum { WS_S, WS_U0, WS_U1 };
inline WsLayout gadget_ws(size_t n, size_t wb, size_t Lt, size_t Ls, bool whole) {
  return whole ? WsLayout(n, wb) : WsLayout(n, wb).blocks(Lt, Ls).blocks(Lt).blocks(Lt);
}
// Hybrid, over the key basis' LE limbs: the raised digits D ([LE][beta c][N]) |
// `pairs` accumulator pairs ([LE][c][N] each: A0 | A1, or a hoisted call's ACC).
enum { WS_D, WS_ACC };
inline WsLayout hybrid_ws(size_t n, size_t wb, size_t LE, size_t beta, size_t pairs = 1) {
  return WsLayout(n, wb).blocks(LE, beta).blocks(LE, 2 * pairs);
}
// A call's own layout is declared in the call (rnt_api.cpp).  The two below are here only so that the CPU test can
// pin them against the expressions they replaced (the second is sized in a wrapper and carved in a helper).
// rnt_ct_mul_relin(_rescale): the tensor's column outputs T (none on the whole-plane rings) | D0 D1 D2 | the gadget
// scratch | the dropped limb's planes LAST0 LAST1 (resc) | the key-switch's diagonal D2H (diag).
enum { MR_T, MR_D, MR_KS, MR_LAST, MR_D2H };
inline WsLayout mul_relin_ws(size_t n, size_t wb, size_t L, size_t nt, bool whole, bool resc, bool diag) {
  return WsLayout(n, wb).blocks(L, nt).blocks(L, 3).sub(gadget_ws(n, wb, L, L, whole)).blocks(1, resc ? 2 : 0)
      .blocks(L, diag ? 1 : 0);
}
// The sums of rotated terms on the four-step key-switch (rnt_ct_linear_bsgs; rnt_ct_linear with ra = rb = a step-0
// term ? 1 : 0 and no `one`): the Montgomery-form plaintexts | the Montgomery one | X0 X1 (the chunk gathered: more
// than one chunk only) | SIG1 | SEED | ra pairs (the baby blocks RB; NT0 NT1) | rb pairs (the inner sums VB; Z0 Z1)
// | the accumulator pairs of one hoisted group HACC (its digits take S) | the gadget scratch.
enum { LF_DM, LF_ONE, LF_X, LF_SIG1, LF_SEED, LF_RA, LF_RB, LF_HACC, LF_KS };
inline WsLayout lin_fused_ws(size_t n, size_t wb, size_t L, size_t dm_bytes, bool one, bool multi, size_t ra,
                             size_t rb, size_t acc_pairs) {
  return WsLayout(n, wb).bytes(dm_bytes).bytes(one ? L * n * wb : 0).blocks(L, multi ? 2 : 0).blocks(L).blocks(L)
      .blocks(L, 2 * ra).blocks(L, 2 * rb).blocks(L, 2 * acc_pairs).sub(gadget_ws(n, wb, L, L, false));
}

}  // namespace rnt
