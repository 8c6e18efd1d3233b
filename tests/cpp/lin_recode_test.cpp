// lin_recode_test.cpp — the host side of the linear maps without a GPU: the recoding of a weight into signed window
// digits (bgn_amd/csrc/linrecode.hpp) and the planning (bgn_amd/csrc/dispatch.hpp plan_lincomb).  For every window width
// 1 .. 8, every w_bits 1 .. 31, the weights at the edges and a few thousand pseudo-random ones: the digits sum to
// sign(w) * (|w| mod 2^w_bits), each lies in [-2^(omega-1), 2^(omega-1)], there are ceil((w_bits+1) / omega) of them,
// and one fits the plane's element.  The plan's table fits the budget it was given, nchunk <= d, forced choices are
// honoured.  Prints "ok"; a violated property prints the case and exits 1.  Built by tests/test_lin_recode_cpu.py with the
// address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>

#include "../../bgn_amd/csrc/dispatch.hpp"
#include "../../bgn_amd/csrc/linrecode.hpp"

using namespace bgn;

static int fails = 0;
#define EXPECT(cond, ...)            \
  do {                               \
    if (!(cond)) {                   \
      printf("FAIL %s: ", #cond);    \
      printf(__VA_ARGS__);           \
      printf("\n");                  \
      ++fails;                       \
    }                                \
  } while (0)

static void check_weight(int32_t w, int w_bits, int omega) {
  int16_t dg[kLinMaxWindows + 1];
  dg[kLinMaxWindows] = 0x5a5a;
  const int nwin = lin_recode(w, w_bits, omega, dg);
  EXPECT(nwin == (w_bits + 1 + omega - 1) / omega && nwin <= kLinMaxWindows, "w_bits %d omega %d: %d windows", w_bits, omega, nwin);
  const long long mag = (long long)(w < 0 ? -(long long)w : (long long)w) % (1ll << w_bits);
  const long long want = w < 0 ? -mag : mag, H = 1ll << (omega - 1);
  long long sum = 0;
  for (int t = nwin - 1; t >= 0; --t) {
    sum = sum * (1ll << omega) + dg[t];
    EXPECT(dg[t] >= -H && dg[t] <= H, "w %d w_bits %d omega %d: digit %d = %d", w, w_bits, omega, t, dg[t]);
    if (lin_digit_bytes(omega) == 1) EXPECT(dg[t] == (int8_t)dg[t], "w %d omega %d: digit %d does not fit a byte", w, omega, dg[t]);
  }
  EXPECT(sum == want, "w %d w_bits %d omega %d: digits give %lld, want %lld", w, w_bits, omega, sum, want);
  EXPECT(nwin == lin_plan_windows(w_bits, omega) && kLinPlanMaxWindow == kLinMaxWindow, "the planner counts %d windows", lin_plan_windows(w_bits, omega));
  EXPECT(dg[kLinMaxWindows] == 0x5a5a, "w %d w_bits %d omega %d: wrote past the windows", w, w_bits, omega);
}

int main() {
  unsigned long long x = 88172645463325252ull;
  size_t n = 0;
  for (int omega = 1; omega <= kLinMaxWindow; ++omega)
    for (int w_bits = 1; w_bits <= 31; ++w_bits) {
      const long long top = (1ll << w_bits) - 1, H = 1ll << (omega - 1);
      const long long edges[] = {0, 1, top, top - 1, top + 1, top + 6, H, H - 1, H + 1, 2 * H - 1, 2 * H, 2 * H + 1,
                                 top - H, top - H + 1, (top + 1) / 2, 0x7fffffffll, 0x78, 0x7f80, 0x80000000ll};
      for (long long e : edges)
        for (int sgn = 1; sgn >= -1; sgn -= 2) {
          if (e > 0x7fffffffll && sgn > 0) continue;                      // INT32_MIN only
          check_weight((int32_t)(sgn * e), w_bits, omega);
          ++n;
        }
      for (int i = 0; i < 40; ++i, ++n) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;                          // xorshift64
        check_weight((int32_t)(x >> 16), w_bits, omega);
      }
    }
  // the plan
  const size_t shapes[][3] = {{1, 1, 1}, {1, 65, 1}, {1, 1, 65}, {2, 3, 7}, {1, 65, 33}, {1, 1024, 1024}, {64, 16, 256},
                              {1, 1, (size_t)1 << 20}, {(size_t)1 << 14, (size_t)1 << 14, (size_t)1 << 14}, {1, (size_t)1 << 28, 1}};
  const size_t budgets[] = {0, 1000, (size_t)1 << 20, (size_t)1 << 30, (size_t)200 << 30};
  for (auto& s : shapes)
    for (size_t budget : budgets)
      for (int level = 1; level <= 2; ++level)
        for (int w_bits : {1, 8, 16, 31})
          for (int64_t fw : {-1, 0, 1, 2, 4, 8, 99})
            for (int64_t fs : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)3, (int64_t)1 << 40}) {
              const size_t eb = level == 1 ? 4 * 36 * 4 + 1 : 2 * 36 * 4;
              const LinPlan p = plan_lincomb(s[0], s[1], s[2], w_bits, budget, eb, level, 65536, fw, fs);
              EXPECT(p.omega >= 1 && p.omega <= 8 && p.nwin == lin_windows(w_bits, p.omega), "omega %d nwin %d", p.omega, p.nwin);
              EXPECT(p.nchunk >= 1 && p.nchunk <= s[2], "%zu x %zu x %zu: nchunk %zu", s[0], s[1], s[2], p.nchunk);
              EXPECT(p.nchunk * s[0] * s[1] <= kMaxBatch, "%zu x %zu x %zu: %zu partials each", s[0], s[1], s[2], p.nchunk);
              EXPECT(p.entries == (p.omega > 1 ? (s[0] * s[2]) << (p.omega - 1) : 0), "entries %zu", p.entries);
              EXPECT(p.entries <= kMaxBatch && p.entries * eb <= budget, "table of %zu entries in a budget of %zu", p.entries, budget);
              if (fw >= 1 && fw <= 8 && budget == (size_t)200 << 30 && s[0] * s[2] <= (size_t)1 << 20) EXPECT(p.omega == fw, "forced window %lld: %d", (long long)fw, p.omega);
              if (fs >= 1) EXPECT(p.nchunk == ((size_t)fs < s[2] ? (size_t)fs : s[2]) || p.nchunk * s[0] * s[1] == kMaxBatch, "forced split %lld: %zu", (long long)fs, p.nchunk);
              ++n;
            }
  EXPECT(plan_lincomb(0, 3, 7, 8, 1 << 20, 100, 1, 65536, -1, -1).omega == 0, "nothing to plan");
  {
    const LinPlan a = plan_lincomb(1, 1024, 1024, 16, (size_t)64 << 30, 577, 1, 65536, -1, -1);
    const LinPlan b = plan_lincomb(1, 1, (size_t)1 << 20, 16, (size_t)64 << 30, 577, 1, 65536, -1, -1);
    printf("1 x 1024 x 1024: omega %d nchunk %zu; 1 x 1 x 2^20: omega %d nchunk %zu\n", a.omega, a.nchunk, b.omega, b.nchunk);
    EXPECT(a.omega > b.omega, "a table shared by 1024 rows is wider than one used once: %d, %d", a.omega, b.omega);
    EXPECT(a.nchunk == 64 && b.nchunk == 65536, "chunks fill the chip: %zu, %zu", a.nchunk, b.nchunk);
  }
  printf("%zu cases\n", n);
  if (fails) return 1;
  printf("ok\n");
  return 0;
}
