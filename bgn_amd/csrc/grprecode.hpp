// grprecode.hpp — balanced-ternary codes of the narrow weights of a linear map taken by column groups (groupops.hpp).
// Free of HIP when a host compiler reads it (tests/cpp/group_plan_test.cpp), __host__ __device__ under hipcc.
//
// A weight counts as s * m with m = |w| mod 2^w_bits, as in linrecode.hpp.  Bit plane t < w_bits of it is the trit
// tau = s * bit_t(m).  The g trits of one plane, one row and one group of g consecutive columns make the code
// c = sum_{i<g} tau_i * 3^i, which lies in [-M, M], M = (3^g - 1) / 2, and fits an int16 for g <= 6 (M = 364).  The table
// of a group holds the entries 1 .. M; the walk adds entry |c|, negated for c < 0.  A column beyond the vector's end
// (the ragged last group) is a zero trit.
//
// The table is built by levels: with k the top non-zero trit of c > 0 (it is +1) and c' = c - 3^k, |c'| <= (3^k - 1) / 2,
//     entry(c) = x_k + sign(c') * entry(|c'|)          (entry(c) = x_k for c' = 0),
// so the 3^k entries of level k read only the group's column k and entries of lower levels.
#pragma once
#include "linrecode.hpp"

namespace bgn {

constexpr int kGrpMaxGroup = 6;      // widest group: 364 entries, codes in an int16
constexpr int kGrpMaxBits = 4;       // widest weights the path takes: one walk over the groups per bit plane

BGN_LIN_HD int grp_pow3(int k) {
  int p = 1;
  for (int i = 0; i < k; ++i) p *= 3;
  return p;
}
BGN_LIN_HD int grp_entries(int g) { return (grp_pow3(g) - 1) / 2; }

// Trit of bit plane t of w.
BGN_LIN_HD int grp_trit(int32_t w, int w_bits, int t) {
  const int b = (int)((lin_magnitude(w, w_bits) >> t) & 1u);
  return w < 0 ? -b : b;
}

// The codes of all planes of the weights w[0 .. n) (n <= g; the missing ones are zero trits): code[t], t < w_bits.
BGN_LIN_HD void grp_codes(const int32_t* w, int n, int w_bits, int16_t* code) {
  for (int t = 0; t < w_bits; ++t) code[t] = 0;
  int p3 = 1;
  for (int i = 0; i < n; ++i, p3 *= 3)
    for (int t = 0; t < w_bits; ++t) code[t] = (int16_t)(code[t] + grp_trit(w[i], w_bits, t) * p3);
}

// The g trits of a code in [-M, M].
BGN_LIN_HD void grp_trits(int c, int g, int* tau) {
  for (int i = 0; i < g; ++i) {
    int r = c % 3;                     // C++ remainder: the sign of c
    if (r < 0) r += 3;
    tau[i] = r == 2 ? -1 : r;
    c = (c - tau[i]) / 3;
  }
}

// Entry c of level k (3^k <= c + (3^k - 1)/2 < 2 * 3^k) is x_k + sign(c') entry(|c'|): c' for the j-th entry of the
// level, j < 3^k, and the entry's own index.
BGN_LIN_HD int grp_level_rest(int k, int j) { return j - (grp_pow3(k) - 1) / 2; }
BGN_LIN_HD int grp_level_entry(int k, int j) { return grp_pow3(k) + grp_level_rest(k, j); }

}  // namespace bgn
