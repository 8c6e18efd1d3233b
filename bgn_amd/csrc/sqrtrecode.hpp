// sqrtrecode.hpp — the public exponent (p + 1) / 4 of the square root in F_p (p = 3 mod 4), recoded once per key into
// the program k_decompress walks (compressops.hpp).  Host only, no HIP: engine.cpp and tests/cpp/sqrt_recode_test.cpp.
//
// Width-3 windows over the odd powers a, a^3, a^5, a^7, each placed so that it ends on a set bit (the exponent is
// public and the same for every lane, so where the windows lie is decided here, not per lane): one product per window
// and none for the zero bits between windows.  An op is one 16-bit word: the low byte says how many squarings come
// first, the high byte which odd power (index (d - 1) / 2 of digit d) is multiplied in afterwards — kSqrtNoMul: none.
// Op 0 has no squarings: the accumulator starts as its power.  Replayed over the integers,
//   v = 0;  for each op: v = (v << squarings) + digit
// gives the exponent back; that is what the test checks.
// For an exponent of b bits: b - (top window's length) squarings and about b / 4 products (a window of three bits and,
// on average, one zero bit behind it), plus one squaring and three products for the table.  At b = 1030: ~1027
// squarings and ~260 products.
#pragma once
#include <stdint.h>

#include <vector>

namespace bgn {

constexpr int kSqrtWindow = 3;                       // 2^(3-1) = 4 odd powers per lane
constexpr int kSqrtPowers = 1 << (kSqrtWindow - 1);
constexpr uint32_t kSqrtNoMul = 0xFF;

// e: little-endian 32-bit words, `bits` its bit length (bit bits-1 is set).
inline std::vector<uint16_t> sqrt_recode(const uint32_t* e, int bits) {
  auto bit = [&](int i) { return (e[i >> 5] >> (i & 31)) & 1u; };
  std::vector<uint16_t> ops;
  uint32_t pending = 0;                              // squarings owed for the zero bits passed over
  auto squarings = [&](uint32_t n) {                 // more than one byte of them: ops without a product in front
    while (n > 255) {
      ops.push_back((uint16_t)((kSqrtNoMul << 8) | 255u));
      n -= 255;
    }
    return n;
  };
  int i = bits - 1;
  while (i >= 0) {
    if (!bit(i)) {
      ++pending;
      --i;
      continue;
    }
    int j = i - kSqrtWindow + 1 > 0 ? i - kSqrtWindow + 1 : 0;
    while (!bit(j)) ++j;                             // the window ends on a set bit: its digit is odd
    uint32_t d = 0;
    for (int k = i; k >= j; --k) d = (d << 1) | bit(k);
    const uint32_t n = ops.empty() ? 0u : squarings(pending + (uint32_t)(i - j + 1));
    ops.push_back((uint16_t)((((d - 1) >> 1) << 8) | n));
    pending = 0;
    i = j - 1;
  }
  if (pending) {
    const uint32_t n = squarings(pending);
    ops.push_back((uint16_t)((kSqrtNoMul << 8) | n));
  }
  return ops;
}

}  // namespace bgn
