// The call-workspace layout type (toy-heaan-ckks_amd/csrc/rnt_ws.hpp) against
// literals worked out by hand, with N = 8 words of 4 bytes (a plane of one
// poly: 32 bytes).  The two call layouts are checked against the expressions
// the calls spelled out before they shared the type:
//   rnt_ct_linear_bsgs  planes = 2 n1 + 2 nv + 4 (+ 2 kHoistT hoisted), used = planes - (one chunk ? 2 : 0),
//                       need = dm + one + used L bc N wb + (L L + 2 L) bc N wb; chunk planes = planes L + L L + 2 L
//   rnt_ct_mul_relin    need = ((nt + 3 + diag) L bc N + ks_words + (resc ? 2 bc N : 0)) wb, ks_words = (L L + 2 L) bc N
// Host code only: no HIP header, no GPU.
#include <cstddef>
#include <cstdio>

#include "rnt_ws.hpp"

using namespace rnt;

static int failures = 0;
#define CHECK(COND)                                         \
  do {                                                      \
    if (!(COND)) {                                          \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #COND); \
      ++failures;                                           \
    }                                                       \
  } while (0)

int main() {
  static char block[8192];
  const size_t n = 8, wb = 4;

  // a flat layout: 100 bytes | 2 blocks of 3 limbs | nothing | 1 block of 1 limb, 5 polys a chunk (160 B a limb)
  {
    WsLayout w = WsLayout(n, wb).bytes(100).blocks(3, 2).blocks(2, 0).blocks(1);
    CHECK(w.planes == 7);  // 3 x 2 + 2 x 0 + 1
    CHECK(w.fixed == 100);
    w.chunk(5);
    CHECK(w.total() == 1220);  // 100 + 2 x 480 + 160
    CHECK(w.total(16) == 1220);
    CHECK(w.pitch(1) == 480 && w.pitch(3) == 160);
    w.place(block);
    CHECK(w.at(0) == block);
    CHECK(w.at(1) == block + 100 && w.at(1, 1) == block + 580);
    CHECK(w.at(2) == nullptr && w.at(2, 1) == nullptr);  // a zero-count part: no address, no bytes
    CHECK(w.at(3) == block + 1060);
    CHECK(w.at(3) + w.pitch(3) == block + w.total());
    CHECK(WsLayout(n, wb).total() == 0 && WsLayout(n, wb).total(16) == 16);
    CHECK(WsLayout(n, wb).bytes(0).place(nullptr).at(0) == nullptr);
  }

  // the gadget scratch, Lt = 2 over Ls = 3: sized for 3 polys, carved for a chunk of 3 and for a last chunk of 1
  {
    const WsLayout sized = gadget_ws(n, wb, 2, 3, false).chunk(3);
    CHECK(sized.planes == 10 && sized.total() == 960);  // (6 + 2 + 2) x 3 x 32
    WsLayout c3 = gadget_ws(n, wb, 2, 3, false).chunk(3).place(block);
    CHECK(c3.at(WS_S) == block && c3.at(WS_U0) == block + 576 && c3.at(WS_U1) == block + 768);
    CHECK(c3.at(WS_U1) + c3.pitch(WS_U1) == block + 960);
    WsLayout c1 = gadget_ws(n, wb, 2, 3, false).chunk(1).place(block);
    CHECK(c1.at(WS_S) == block && c1.at(WS_U0) == block + 192 && c1.at(WS_U1) == block + 256);  // contiguous at 32 B
    CHECK(c1.at(WS_U1) + c1.pitch(WS_U1) == block + 320 && c1.total() <= sized.total());
    CHECK(gadget_ws(n, wb, 2, 3, true).slots == 0 && gadget_ws(n, wb, 2, 3, true).total() == 0);
    // nested: no bytes, no address on the whole-plane rings
    WsLayout outer = WsLayout(n, wb).bytes(64).sub(gadget_ws(n, wb, 2, 3, true)).chunk(3).place(block);
    CHECK(outer.total() == 64 && outer.at(1) == nullptr);
    WsLayout outer2 = WsLayout(n, wb).bytes(64).sub(sized).blocks(1).chunk(3).place(block);
    CHECK(outer2.planes == 11 && outer2.total() == 64 + 960 + 96);
    CHECK(outer2.at(1) == block + 64 && outer2.at(2) == block + 1024);
  }

  // the hybrid scratch, LE = 4, beta = 2, two accumulator pairs (a hoisted group of two steps)
  {
    const WsLayout sized = hybrid_ws(n, wb, 4, 2, 2).chunk(3);
    CHECK(sized.planes == 24 && sized.total() == 2304);  // (4 x 2 + 4 x 4) x 3 x 32
    CHECK(hybrid_ws(n, wb, 4, 2).planes == 16);          // D | A0 | A1: LE beta + 2 LE
    WsLayout c3 = hybrid_ws(n, wb, 4, 2, 2).chunk(3).place(block);
    CHECK(c3.at(WS_D) == block && c3.at(WS_ACC) == block + 768 && c3.at(WS_ACC, 1) == block + 1152);
    CHECK(c3.at(WS_ACC, 3) + c3.pitch(WS_ACC) == block + 2304);
    WsLayout c1 = hybrid_ws(n, wb, 4, 2, 2).chunk(1).place(block);
    CHECK(c1.at(WS_D) == block && c1.at(WS_ACC) == block + 256 && c1.at(WS_ACC, 1) == block + 384);
    CHECK(c1.at(WS_ACC, 3) + c1.pitch(WS_ACC) == block + 768 && c1.total() <= sized.total());
  }

  // rnt_ct_linear_bsgs on the four-step key-switch: L = 3, n1 = 2, nv = 2, n2 = 2 (4 plaintexts), chunks of 2.
  // dm = 3 x 4 x 32 = 384, one = 96, a chunk block 3 x 2 x 32 = 192, the gadget scratch 15 x 2 x 32 = 960
  {
    const size_t L = 3, dm = 384, kHoistT = 4;
    struct {
      bool multi, hoisted;
      size_t need;
    } want[] = {{true, false, 3744},   // 480 + 12 x 192 + 960
                {false, false, 3360},  // 480 + 10 x 192 + 960
                {true, true, 5280},    // 480 + 20 x 192 + 960
                {false, true, 4896}};  // 480 + 18 x 192 + 960
    for (const auto& c : want) {
      WsLayout w = lin_fused_ws(n, wb, L, dm, true, c.multi, 2, 2, c.hoisted ? kHoistT : 0).chunk(2).place(block);
      CHECK(w.total() == c.need);
      CHECK(w.at(LF_DM) == block && w.at(LF_ONE) == block + 384);
      const size_t x = c.multi ? 384 : 0;
      CHECK(w.at(LF_X) == (c.multi ? block + 480 : nullptr) && w.at(LF_X, 1) == (c.multi ? block + 672 : nullptr));
      CHECK(w.at(LF_SIG1) == block + 480 + x && w.at(LF_SEED) == block + 672 + x);
      CHECK(w.at(LF_RA) == block + 864 + x && w.at(LF_RA, 3) == block + 1440 + x);
      CHECK(w.at(LF_RB) == block + 1632 + x && w.pitch(LF_RB) == 192);
      CHECK(w.at(LF_HACC) == (c.hoisted ? block + 2400 + x : nullptr));
      CHECK(w.at(LF_KS) == block + 2400 + x + (c.hoisted ? 1536 : 0));
      CHECK(w.at(LF_KS) + 960 == block + w.total());
    }
    // the chunk rule counts the two gather blocks whatever the chunk: planes L + L L + 2 L
    CHECK(lin_fused_ws(n, wb, L, dm, true, true, 2, 2, 0).planes == 51);        // 12 x 3 + 15
    CHECK(lin_fused_ws(n, wb, L, dm, true, true, 2, 2, kHoistT).planes == 75);  // 20 x 3 + 15
    // rnt_ct_linear on the same layout: no `one`, NT0 NT1 Z0 Z1 with a step-0 term: dm + (2 + 2 + 4) x 192 + 960
    CHECK(lin_fused_ws(n, wb, L, dm, false, true, 1, 1, 0).chunk(2).total() == 384 + 1536 + 960);
    CHECK(lin_fused_ws(n, wb, L, dm, false, false, 0, 0, 0).chunk(2).total() == 384 + 384 + 960);
  }

  // rnt_ct_mul_relin(_rescale): L = 3, chunks of 2: a chunk block 192, the gadget scratch 960, LAST0 | LAST1 128
  {
    const size_t L = 3;
    struct {
      size_t nt;
      bool resc, diag;
      size_t need;
    } want[] = {{0, false, false, 1536}, {0, true, false, 1664}, {0, false, true, 1728}, {0, true, true, 1856},
                {1, false, false, 1728}, {1, true, false, 1856}, {1, false, true, 1920}, {1, true, true, 2048},
                {4, false, false, 2304}, {4, true, false, 2432}, {4, false, true, 2496}, {4, true, true, 2624}};
    for (const auto& c : want) {
      WsLayout w = mul_relin_ws(n, wb, L, c.nt, false, c.resc, c.diag).chunk(2).place(block);
      CHECK(w.total() == c.need);
      const size_t t = c.nt * 192;
      CHECK(w.at(MR_T) == (c.nt ? block : nullptr));
      CHECK(w.at(MR_D, 0) == block + t && w.at(MR_D, 1) == block + t + 192 && w.at(MR_D, 2) == block + t + 384);
      CHECK(w.at(MR_KS) == block + t + 576);
      CHECK(w.at(MR_LAST, 0) == (c.resc ? block + t + 1536 : nullptr));
      CHECK(w.at(MR_LAST, 1) == (c.resc ? block + t + 1600 : nullptr));
      CHECK(w.at(MR_D2H) == (c.diag ? block + t + 1536 + (c.resc ? 128 : 0) : nullptr));  // after LAST with resc alone
    }
    CHECK(mul_relin_ws(n, wb, L, 4, false, true, true).chunk(2).place(block).at(MR_T, 3) == block + 576);
    CHECK(mul_relin_ws(n, wb, L, 0, true, false, false).chunk(2).total() == 576);  // the whole-plane rings: D0 D1 D2
  }

  std::printf(failures ? "FAILED (%d failures)\n" : "OK (%d failures)\n", failures);
  return failures ? 1 : 0;
}
