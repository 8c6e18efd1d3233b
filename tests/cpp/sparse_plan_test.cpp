// sparse_plan_test.cpp — dispatch.hpp plan_sparse_lincomb without a GPU: 1 <= nchunk <= min(row_max, nnz) (1 for an empty
// structure) and at most 2^28 partials, the window narrowed until its table fits the budget, forced lin_window / lin_split
// honoured, and window 1 when no column is shared (nnz <= d).  Prints "ok", or the violated property and exits 1.  Built
// by tests/test_abi_sparse_lincomb_cpu.py with the address and UB sanitizers.
#include <cstdio>

#include "../../bgn_amd/csrc/dispatch.hpp"

using namespace bgn;

static int fails = 0;
#define EXPECT(cond) \
  do { if (!(cond)) { printf("FAIL %s: %zu x %zu x %zu nnz %zu row_max %zu w_bits %d budget %zu level %d forced %lld / %lld\n", #cond, nvec, nrows, d, nnz, row_max, w_bits, budget, level, (long long)fw, (long long)fs); ++fails; } } while (0)

static void check(size_t nvec, size_t nrows, size_t d, size_t nnz, size_t row_max, int w_bits, size_t budget, int level,
                  int64_t fw, int64_t fs) {
  const size_t eb = level == 1 ? 577 : 288, chip = level == 1 ? 65536 : 131072;
  const LinPlan p = plan_sparse_lincomb(nvec, nrows, d, nnz, row_max, w_bits, budget, eb, level, chip, fw, fs);
  const size_t rm = row_max < nnz ? row_max : nnz, nout = nvec * nrows;
  EXPECT(p.nchunk >= 1 && p.nchunk <= (rm ? rm : 1) && p.nchunk * nout <= ((size_t)1 << 28));
  EXPECT(p.omega >= 1 && p.omega <= 8 && p.nwin == (w_bits + p.omega) / p.omega);
  EXPECT(p.entries == (p.omega > 1 ? (nvec * d) << (p.omega - 1) : 0));
  EXPECT(p.entries <= ((size_t)1 << 28) && p.entries * eb <= (p.entries ? budget : p.entries * eb));      // the table fits
  if (fs >= 1 && (size_t)fs <= rm && (size_t)fs * nout <= ((size_t)1 << 28)) EXPECT(p.nchunk == (size_t)fs);
  if (fw >= 1) {                                                    // the forced window, or the widest below it that fits
    const int want = fw > 8 ? 8 : (int)fw;
    EXPECT(p.omega <= want);
    if (p.omega < want) EXPECT(((nvec * d) << p.omega) > ((size_t)1 << 28) || ((nvec * d) << p.omega) * eb > budget);
  } else if (nnz <= d) {
    EXPECT(p.omega == 1);                                           // no column is shared: no table
  }
}

int main() {
  const size_t shapes[][5] = {{1, 1, 1, 0, 0}, {1, 1, 1, 1, 1}, {2, 70, 37, 280, 8}, {1, 300, 302, 900, 3}, {1, 3, 50, 201, 200},
                              {1, (size_t)1 << 20, ((size_t)1 << 20) + 15, (size_t)1 << 24, 16}, {1, 1024, 1024, 16384, 16},
                              {1, 4096, (size_t)1 << 20, (size_t)1 << 20, 256}, {1, 2, (size_t)1 << 20, (size_t)1 << 21, (size_t)1 << 40},
                              {(size_t)1 << 14, (size_t)1 << 14, 5, 1000, (size_t)1 << 20}, {1, 1, (size_t)1 << 28, (size_t)1 << 28, 7}};
  const size_t budgets[] = {0, 1000, (size_t)1 << 20, (size_t)1 << 30, (size_t)64 << 30};
  const int64_t forced[] = {-1, 0, 1, 3, 4, 8, 200, (int64_t)1 << 40};
  for (const auto& s : shapes)
    for (int w_bits : {1, 7, 16, 31})
      for (size_t budget : budgets)
        for (int level : {1, 2})
          for (int64_t fw : forced)
            for (int64_t fs : forced) check(s[0], s[1], s[2], s[3], s[4], w_bits, budget, level, fw, fs);
  // a shared column earns a table when the budget allows, and the skew bound cuts a giant row although the chip is full
  if (plan_sparse_lincomb(1, 1024, 1024, 16384, 16, 16, (size_t)64 << 30, 577, 1, 65536, -1, -1).omega < 2) ++fails;
  if (plan_sparse_lincomb(1, (size_t)1 << 17, 64, (size_t)1 << 20, (size_t)1 << 20, 8, 0, 577, 1, 65536, -1, -1).nchunk != 1024) ++fails;
  if (plan_sparse_lincomb(0, 3, 7, 5, 5, 8, 1 << 20, 577, 1, 65536, -1, -1).omega != 0) ++fails;
  printf(fails ? "failed\n" : "ok\n");
  return fails ? 1 : 0;
}
