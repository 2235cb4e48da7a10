// The streaming launchers' shared geometry (toy-heaan-ckks_amd/csrc/rnt_launch.hpp)
// against literals worked out by hand from the formulas each launcher used to
// spell out for itself:
//   vec  = N % V == 0 && every stride % V == 0 && (OR of the pointers) % 16 == 0, V = 16 / sizeof(W)
//   bx   = ((vec ? words / V : words) + 255) / 256, for xcd_gid() then (bx + 7) & ~7
//   bx > 0x7fffffff or y > 65535: refused
//   runs = min(limbs, max(1024 / blocks, 1)), per = ceil(limbs / runs), extent = ceil(limbs / per)
//   tier = the first T with n <= T, the last tier for every other n
// Host code only: no HIP header, no GPU.
#include <cstdint>
#include <cstdio>

#include "rnt_launch.hpp"

using namespace rnt;

static int failures = 0;
#define CHECK(COND)                                         \
  do {                                                      \
    if (!(COND)) {                                          \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #COND); \
      ++failures;                                           \
    }                                                       \
  } while (0)

template <int... Ts>
static int tier(uint64_t n) {
  return with_tier<Ts...>(n, [](auto T) { return (int)decltype(T)::value; });
}

struct FakeTables {
  int wide;
};
struct FakeLaunch {
  const FakeTables* t;
};

int main() {
  const void* a16 = (const void*)(uintptr_t)0x1000;
  const void* b16 = (const void*)(uintptr_t)0x2340;
  const void* p4 = (const void*)(uintptr_t)0x1004;
  const void* p8 = (const void*)(uintptr_t)0x1008;
  const void* none = nullptr;
  const uint64_t N = 1024;

  // vec: alignment of pointers, strides and the run
  CHECK(!vec_ok<uint32_t>(N, {N}, ptr_bits(a16, p4)));  // a u32 buffer one word off
  CHECK(!vec_ok<uint64_t>(N, {N}, ptr_bits(p8, b16)));  // a u64 buffer one word off
  CHECK(!vec_ok<uint32_t>(N, {N, N + 1}, ptr_bits(a16, b16)));
  CHECK(!vec_ok<uint64_t>(N, {N + 1}, ptr_bits(a16, b16)));
  CHECK(vec_ok<uint32_t>(N, {N, 0}, ptr_bits(a16, none, b16)));  // a null optional pointer, its stride 0
  CHECK(vec_ok<uint32_t>(N, {N, 4 * N}, ptr_bits(a16, b16)));
  CHECK(vec_ok<uint64_t>(N, {N, 2 * N}, ptr_bits(a16, b16)));
  CHECK(vec_ok<uint32_t>(N, {}, ptr_bits(a16)));
  CHECK(!vec_ok<uint32_t>(2, {}, ptr_bits(a16)));  // N = 2: half a u32 vector
  CHECK(vec_ok<uint64_t>(2, {}, ptr_bits(a16)));   //        one u64 vector
  CHECK(!vec_ok<uint32_t>(1026, {}, ptr_bits(a16)));  // elementwise: a limb's words, 1026 % 4 = 2
  CHECK(ptr_bits(none) == 0 && ptr_bits(a16, p4) % 16 == 4 && ptr_bits(p8, none) % 16 == 8);
  // moddown_auto: a word-aligned output decides nothing while it stays out of the pointers
  CHECK(vec_ok<uint32_t>(N, {N}, ptr_bits(a16, none)));
  CHECK(!vec_ok<uint32_t>(N, {N}, ptr_bits(a16, none, p4)));

  // bx
  CHECK(blocks_x<uint32_t>(256, false) == 1);
  CHECK(blocks_x<uint32_t>(257, false) == 2);
  CHECK(blocks_x<uint64_t>(257, false) == 2);
  CHECK(blocks_x<uint32_t>(1024, true) == 1);  // 256 vectors of 4 words
  CHECK(blocks_x<uint64_t>(1024, true) == 2);  // 512 vectors of 2 words
  CHECK(blocks_x<uint32_t>(1, false) == 1);
  CHECK(blocks_x<uint32_t>(256, false, true) == 8);    // 1 block
  CHECK(blocks_x<uint32_t>(2048, false, true) == 8);   // 8 blocks
  CHECK(blocks_x<uint32_t>(2049, false, true) == 16);  // 9 blocks
  CHECK(blocks_x<uint32_t>(8192, true, true) == 8);    // 2048 vectors: 8 blocks
  CHECK(blocks_x<uint32_t>(0x7fffffffull * 256, false) == 0x7fffffffull);
  CHECK(blocks_x<uint32_t>(0x7fffffffull * 256 + 1, false) == 0x80000000ull);
  CHECK(grid_ok(0x7fffffffull));
  CHECK(!grid_ok(0x80000000ull));
  CHECK(grid_ok(1, 65535));
  CHECK(!grid_ok(1, 65536));
  CHECK(!grid_ok(0x80000000ull, 1));

  // limb split: {blocks, limbs} -> runs, per, extent
  CHECK(kSplitBlocks == 1024);
  LimbSplit s = limb_split(5, 1);
  CHECK(s.runs == 5 && s.per == 1 && s.extent == 5);
  s = limb_split(5, 300);  // (modup: bx 100 x beta 3; lincomb: 2 x bx 150)
  CHECK(s.runs == 3 && s.per == 2 && s.extent == 3);
  s = limb_split(5, 600);
  CHECK(s.runs == 1 && s.per == 5 && s.extent == 1);
  s = limb_split(5, 2048);
  CHECK(s.runs == 1 && s.per == 5 && s.extent == 1);
  s = limb_split(1, 1);
  CHECK(s.runs == 1 && s.per == 1 && s.extent == 1);
  s = limb_split(7, 256);  // 1024 / 256 = 4 runs: 2 limbs each, 4 rows (the last with one)
  CHECK(s.runs == 4 && s.per == 2 && s.extent == 4);
  s = limb_split(9, 128);  // 8 runs: 2 limbs each, 5 rows
  CHECK(s.runs == 8 && s.per == 2 && s.extent == 5);

  // tiers
  CHECK((tier<4, 8, 16, 0>(4) == 4));
  CHECK((tier<4, 8, 16, 0>(5) == 8));
  CHECK((tier<4, 8, 16, 0>(16) == 16));
  CHECK((tier<4, 8, 16, 0>(17) == 0));
  CHECK((tier<4, 8, 16, 0>(1) == 4));
  CHECK((tier<4, 8, 0>(8) == 8));
  CHECK((tier<4, 8, 0>(9) == 0));
  CHECK((tier<4, 8, 16>(16) == 16));
  CHECK((tier<4, 8, 16>(9) == 16));
  CHECK((tier<1, 2, 3, 4>(1) == 1));
  CHECK((tier<1, 2, 3, 4>(3) == 3));
  CHECK((tier<1, 2, 3, 4>(4) == 4));
  CHECK((tier<0, 1, 2, 3, 4>(0) == 0));  // the elementwise ops: 0 .. 3, any other 4
  CHECK((tier<0, 1, 2, 3, 4>(3) == 3));
  CHECK((tier<0, 1, 2, 3, 4>((unsigned)-1) == 4));
  CHECK((tier<0, 1>(0) == 0 && tier<0, 1>(7) == 1));

  // flags and word types
  CHECK(with_bool(true, [](auto B) { return decltype(B)::value ? 1 : 2; }) == 1);
  CHECK(with_bool(false, [](auto B) { return decltype(B)::value ? 1 : 2; }) == 2);
  const FakeTables t32{0}, t64{1};
  CHECK(by_word(FakeLaunch{&t32}, [](auto w) { return sizeof(w); }) == 4);
  CHECK(by_word(FakeLaunch{&t64}, [](auto w) { return sizeof(w); }) == 8);

  std::printf("%s (%d failures)\n", failures ? "FAIL" : "OK", failures);
  return failures ? 1 : 0;
}
