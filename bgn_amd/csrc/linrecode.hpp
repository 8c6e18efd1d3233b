// linrecode.hpp — signed window digits of the plaintext weights of a linear map (linops.hpp).  Free of HIP when a host
// compiler reads it (tests/cpp/lin_recode_test.cpp), __host__ __device__ under hipcc.
//
// A weight is the integer sign(w) * (|w| mod 2^w_bits), 1 <= w_bits <= 31.  Its magnitude m is cut into windows of
// `omega` bits from the low end: dg = v mod 2^omega; if dg > H = 2^(omega-1) then dg -= 2^omega and the next window
// takes a carry.  The sign of w is applied to every digit, so a digit lies in [-H, H] and the walk needs the multiples
// 1 .. H of a ciphertext only.  The comparison is `>`, not `>=`: the top window of the ceil((w_bits + 1) / omega)
// windows holds at most omega - 1 bits of m, so with the carry it reaches H at most and never carries out; with `>=` it
// would (omega = 4, w_bits = 7, m = 0x78), and omega = 1 would carry for ever.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BGN_LIN_HD __host__ __device__ inline
#else
#define BGN_LIN_HD inline
#endif

namespace bgn {

constexpr int kLinMaxWindow = 8;     // widest window: 128 multiples per ciphertext
constexpr int kLinMaxWindows = 32;   // omega = 1, w_bits = 31

BGN_LIN_HD int lin_windows(int w_bits, int omega) { return (w_bits + omega) / omega; }      // ceil((w_bits + 1) / omega)

BGN_LIN_HD uint32_t lin_magnitude(int32_t w, int w_bits) {
  const uint32_t a = w < 0 ? 0u - (uint32_t)w : (uint32_t)w;                               // |INT32_MIN| = 2^31 fits
  return a & ((1u << w_bits) - 1u);
}

// Digit t of w, t < lin_windows(w_bits, omega), into dg[t]; returns the number of windows.
BGN_LIN_HD int lin_recode(int32_t w, int w_bits, int omega, int16_t* dg) {
  const int nwin = lin_windows(w_bits, omega);
  const int32_t H = 1 << (omega - 1);
  const uint32_t mask = (1u << omega) - 1u;
  uint32_t v = lin_magnitude(w, w_bits);
  for (int t = 0; t < nwin; ++t) {
    int32_t d = (int32_t)(v & mask);
    v >>= omega;
    if (d > H) {
      d -= 2 * H;
      v += 1;
    }
    dg[t] = (int16_t)(w < 0 ? -d : d);
  }
  return nwin;
}

// A digit plane holds one digit per (column, row).  Digits of windows up to 7 bits fit an int8; at omega = 8 the range
// [-128, 128] has 257 values and the plane holds int16.
BGN_LIN_HD int lin_digit_bytes(int omega) { return omega == 8 ? 2 : 1; }

}  // namespace bgn
