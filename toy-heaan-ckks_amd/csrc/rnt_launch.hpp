// rnt_launch.hpp -- the launch geometry every streaming launcher shares, and
// compile-time dispatch of run-time choices.  Host only and free of the HIP
// headers (tests/cpp/test_launch_geom.cpp compiles it alone): a launcher turns
// a refused geometry into its own error code.
//
// A streaming kernel<W, VEC, ...> runs 256 lanes a workgroup over the words of
// a limb: grid x = blocks of lanes, a lane owning V = 16 / sizeof(W) words
// (VEC: 16-byte accesses) or one word; y (or z) = limbs, or runs of limbs.
#pragma once
#include <algorithm>
#include <cstdint>
#include <initializer_list>
#include <type_traits>

namespace rnt {

// The address bits of any number of pointers (a null pointer adds none).
template <class... P>
uintptr_t ptr_bits(P... p) {
  return (uintptr_t(0) | ... | (uintptr_t)p);
}

// Whether 16-byte accesses serve: whole vectors within a run of n words, every
// stride (in words; 0 for one that goes with a null pointer) a whole number of
// vectors, every non-null pointer of `bits` 16-byte aligned.
template <class W>
bool vec_ok(uint64_t n, std::initializer_list<uint64_t> strides, uintptr_t bits) {
  constexpr uint64_t V = 16 / sizeof(W);
  for (uint64_t s : strides)
    if (s % V != 0) return false;
  return n % V == 0 && bits % 16 == 0;
}

// Grid x: 256-lane blocks over `words` (over its 16-byte vectors where vec),
// rounded up to a multiple of 8 for the kernels that deal blocks to the XCDs
// (xcd_gid()).
template <class W>
uint64_t blocks_x(uint64_t words, bool vec, bool round8 = false) {
  const uint64_t bx = ((vec ? words / (16 / sizeof(W)) : words) + 255) / 256;
  return round8 ? (bx + 7) & ~7ull : bx;
}
// The hardware's grid limits: x, and y or z where a launcher puts limbs there.
inline bool grid_ok(uint64_t bx, uint64_t y = 0) { return bx <= 0x7fffffffull && y <= 65535; }

// Workgroups from which a grid over the vectors alone fills the 256 CUs.
constexpr uint64_t kSplitBlocks = 1024;
// Runs of limbs per lane: all `limbs` in one lane where `blocks` workgroups
// fill the device already, else split into `extent` grid rows of `per` limbs.
struct LimbSplit {
  uint64_t runs;
  uint32_t per, extent;
};
inline LimbSplit limb_split(uint64_t limbs, uint64_t blocks) {
  LimbSplit s;
  s.runs = std::min<uint64_t>(limbs, std::max<uint64_t>(kSplitBlocks / blocks, 1));
  s.per = (uint32_t)((limbs + s.runs - 1) / s.runs);
  s.extent = (uint32_t)((limbs + s.per - 1) / s.per);
  return s;
}

// f(std::bool_constant<flag>{}).
template <class F>
auto with_bool(bool flag, F&& f) {
  return flag ? f(std::true_type{}) : f(std::false_type{});
}
// f(std::integral_constant<int, T>{}) for the first tier T with n <= T; the last
// tier takes every n (0: a kernel's form without a register tier).
template <int T, int... Ts, class F>
auto with_tier(uint64_t n, F&& f) {
  if constexpr (sizeof...(Ts) == 0) return f(std::integral_constant<int, T>{});
  else return n <= (uint64_t)T ? f(std::integral_constant<int, T>{}) : with_tier<Ts...>(n, f);
}
// f(W{}) with W the word type of k's basis: uint32_t, or uint64_t where wide.
template <class K, class F>
auto by_word(const K& k, F&& f) {
  return k.t->wide ? f(uint64_t{}) : f(uint32_t{});
}

}  // namespace rnt
