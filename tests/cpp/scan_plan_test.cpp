// scan_plan_test.cpp — dispatch.hpp plan_scan without a GPU: the recursion ends with one chunk per segment, every level's
// chunks cover its segments exactly once, c >= 2 wherever a segment has two elements, a level scans exactly the totals
// of the level above, the workspace bound holds, a forced chunk is honoured on the first level only.  Prints "ok", or
// the violated property and exits 1.  Built by tests/test_abi_scan_cpu.py with the address and UB sanitizers.
#include <cstdio>

#include "../../bgn_amd/csrc/dispatch.hpp"

using namespace bgn;

static int fails = 0;
#define EXPECT(cond) \
  do { if (!(cond)) { printf("FAIL %s: %zu x %zu forced %lld run %lld bound %zu level %d\n", #cond, nseg, len, (long long)forced, (long long)run_min, bound, k); ++fails; } } while (0)

static void check(size_t nseg, size_t len, int64_t forced, int64_t run_min, size_t bound) {
  const ScanPlan p = plan_scan(nseg, len, 65536, run_min, forced, bound);
  const size_t eb = bound == 1 ? 2 : bound;      // (a bound of 1 would not let the recursion shrink: taken as 2)
  int k = -1;
  EXPECT(p.levels >= 1 && p.levels <= 32);
  size_t cur = len;
  for (k = 0; k < p.levels && k < 32; ++k) {
    const size_t c = p.c[k], nch = p.nch[k];
    EXPECT(p.len[k] == cur);                                         // this level scans the totals of the one above
    EXPECT(c >= 1 && c <= cur && (c >= 2 || cur == 1));
    EXPECT(nch >= 1 && (nch - 1) * c < cur && nch * c >= cur);       // nch chunks, the last one of 1 .. c elements
    EXPECT(!eb || c <= eb);
    EXPECT((nch == 1) == (k + 1 == p.levels));
    if (k == 0 && forced >= 2 && (size_t)forced <= cur && (!eb || (size_t)forced <= eb)) EXPECT(c == (size_t)forced);
    if (k > 0) EXPECT(plan_scan(nseg, cur, 65536, run_min, -1, bound).c[0] == c);     // planned, whatever was forced above
    cur = nch;
  }
}

int main() {
  const size_t lens[] = {1, 2, 3, 7, 16, 17, 64, 65, 130, 257, 600, 5000, 65537, (size_t)1 << 20, (size_t)1 << 28};
  const size_t segs[] = {1, 3, 257, 65536, 65537, (size_t)1 << 28};
  const int64_t forced[] = {-1, 0, 1, 2, 7, 64, (int64_t)1 << 40};
  const int64_t runs[] = {4, 2, 0, -5, 1000};
  const size_t bounds[] = {0, 1, 2, 37};
  for (size_t len : lens)
    for (size_t nseg : segs)
      for (int64_t f : forced)
        for (int64_t r : runs)
          for (size_t b : bounds)
            if (len <= (((size_t)1 << 28) / nseg)) check(nseg, len, f, r, b);
  if (plan_scan(0, 5, 65536, 4, -1, 0).levels != 0 || plan_scan(1, 600, 65536, 4, 2, 0).levels < 4) ++fails;
  printf(fails ? "failed\n" : "ok\n");
  return fails ? 1 : 0;
}
