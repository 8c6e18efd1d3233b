// bucket_plan_test.cpp — dispatch.hpp plan_lincomb_buckets without a GPU: forced values clamped to what the kernels accept,
// the run bound nrows * nwin * (ceil(d/R) + H) and the pass count covering every admissible (d, R, window) without
// overflow up to d = 2^28, never planned below the floor, planned for 1 x 1 x 2^20 at 16-bit weights on both levels, and
// an estimate that does not fall as nrows grows.  Prints "ok", or the violated property and exits 1.  Built by
// tests/test_bucket_plan_cpu.py with the address and UB sanitizers.
#include <cstdio>

#include "../../bgn_amd/csrc/dispatch.hpp"

using namespace bgn;

static int fails = 0;
#define EXPECT(cond) \
  do { if (!(cond)) { printf("FAIL %s: %zu x %zu x %zu w_bits %d level %d forced %lld / %lld / %lld\n", #cond, nvec, nrows, d, w_bits, level, (long long)fb, (long long)fw, (long long)fr); ++fails; } } while (0)

static const size_t kBudget = (size_t)64 << 30;

static BktPlan plan(size_t nvec, size_t nrows, size_t d, int w_bits, int level, int64_t fb, int64_t fw, int64_t fr,
                    size_t budget = kBudget) {
  return plan_lincomb_buckets(nvec, nrows, d, w_bits, budget, level == 1 ? 577 : 288, 289, level, 65536, -1, -1, fb, fw, fr);
}

static void check(size_t nvec, size_t nrows, size_t d, int w_bits, int level, int64_t fb, int64_t fw, int64_t fr) {
  const BktPlan p = plan(nvec, nrows, d, w_bits, level, fb, fw, fr);
  if (fb == 0) EXPECT(!p.use);
  if (fb < 0 && d < kBktMinCols) EXPECT(!p.use);                      // the floor
  if (!p.use) return;
  const size_t H = (size_t)1 << (p.omega - 1), R = p.R;
  EXPECT(p.omega >= 1 && p.omega <= 8 && p.nwin == (w_bits + p.omega) / p.omega && p.nwin * H <= 512);
  EXPECT(R >= 2 && R <= 256);
  if (fw >= 1) EXPECT(p.omega == (fw > 8 ? 8 : (int)fw));
  if (fr >= 1) EXPECT(R == (size_t)(fr < 2 ? 2 : fr > 256 ? 256 : fr));
  EXPECT(p.nb == nrows * p.nwin * H && p.nc == (int)((H + 15) / 16));
  // the passes leave at most one element per bucket, and fit the plan's arrays
  size_t len = d;
  int passes = 0;
  do { len = (len + R - 1) / R; ++passes; } while (len > 1);
  EXPECT(p.npass == passes && p.npass <= kBktMaxPasses);
  // the bound covers the runs of ANY distribution of the columns: sum_b ceil(c_b / R) <= ceil(d / R) + H per window
  EXPECT(p.nruns[0] == nrows * p.nwin * ((d + R - 1) / R + H));
  for (int k = 1; k < p.npass; ++k) EXPECT(p.nruns[k] >= (p.nruns[k - 1] + R - 1) / R + p.nb);
  for (int k = 0; k < p.npass; ++k) EXPECT(p.nruns[k] <= p.cap[k & 1]);
  EXPECT(p.cap[0] >= p.nb && p.cap[1] >= p.nb);                       // the fold's stages
  EXPECT(p.nruns[0] * R <= 0xffffffffu);                              // 32-bit cursors
  EXPECT(nvec * p.cap[0] <= ((size_t)1 << 28) && nvec * p.cap[1] <= ((size_t)1 << 28));
  EXPECT(p.bytes <= kBudget && p.bytes >= p.nruns[0] * R * 4 + nvec * (p.cap[0] + p.cap[1]) * 289);
}

int main() {
  const size_t shapes[][3] = {{1, 1, 1}, {1, 1, 67}, {2, 3, 67}, {1, 2, 300}, {1, 1, 1023}, {1, 1, 1024}, {1, 1, (size_t)1 << 20},
                              {1, 4, (size_t)1 << 18}, {1, 64, (size_t)1 << 14}, {1, 1024, 1024}, {3, 5, 100001},
                              {1, (size_t)1 << 18, 1024}, {1, 1, (size_t)1 << 28}, {(size_t)1 << 10, 1, (size_t)1 << 18}};
  const int64_t forced[] = {-1, 0, 1, 2, 3, 4, 8, 16, 200, 300, (int64_t)1 << 40};
  for (const auto& s : shapes)
    for (int w_bits : {1, 8, 16, 31})
      for (int level : {1, 2})
        for (int64_t fb : {-1, 0, 1})
          for (int64_t fw : forced)
            for (int64_t fr : forced) check(s[0], s[1], s[2], w_bits, level, fb, fw, fr);
  for (int level : {1, 2}) {
    if (!plan(1, 1, (size_t)1 << 20, 16, level, -1, -1, -1).use) { printf("FAIL not planned for 1 x 1 x 2^20, level %d\n", level); ++fails; }
    if (plan(1, 1, (size_t)1 << 20, 16, level, 1, -1, -1, 1000).use) { printf("FAIL used without the memory\n"); ++fails; }
    for (size_t d : {(size_t)1024, (size_t)1 << 14, (size_t)1 << 18}) {      // the estimate does not fall as nrows grows
      double last = 0;
      for (size_t nrows = 1; nrows * d <= ((size_t)1 << 28) && nrows <= 4096; nrows *= 2) {
        const BktPlan p = plan(1, nrows, d, 16, level, 1, -1, -1);
        if (!p.use || p.cost < last) { printf("FAIL estimate falls: level %d d %zu nrows %zu\n", level, d, nrows); ++fails; }
        last = p.cost;
      }
    }
  }
  printf(fails ? "failed\n" : "ok\n");
  return fails ? 1 : 0;
}
