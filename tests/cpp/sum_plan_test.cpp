// sum_plan_test.cpp — the planning of segmented sums (bgn_amd/csrc/dispatch.hpp plan_sum) without a GPU: for a grid of
// (nseg, seg_len, forced split, shortest run) the passes terminate with split 1, no split exceeds the length it
// divides, a forced first split is honoured (clamped to the length), and the strided walk of every pass —
// lane t takes t, t + split, ... — visits every element of a segment exactly once.  Prints one line per configuration
// class and "ok"; a violated property prints the case and exits 1.  Built by tests/test_sum_plan_cpu.py with the
// address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../bgn_amd/csrc/dispatch.hpp"

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

static void walk_covers(size_t len, size_t split) {
  // split * ceil(len / split) slots, of which exactly the first len are elements: each visited once
  const size_t steps = (len + split - 1) / split;
  std::vector<unsigned char> seen(len, 0);
  size_t visited = 0;
  for (size_t t = 0; t < split; ++t)
    for (size_t j = 0; j < steps; ++j) {
      const size_t e = j * split + t;
      if (e >= len) continue;
      EXPECT(!seen[e], "len %zu split %zu element %zu twice", len, split, e);
      seen[e] = 1;
      ++visited;
    }
  EXPECT(visited == len, "len %zu split %zu visited %zu", len, split, visited);
  EXPECT(split * steps >= len && split * (steps - 1) < len, "len %zu split %zu steps %zu", len, split, steps);
}

static SumPlan check(size_t nseg, size_t len, int64_t forced, int64_t run_min, size_t chip) {
  const SumPlan p = plan_sum(nseg, len, chip, forced, run_min);
  EXPECT(p.passes >= 1 && p.passes <= 32, "nseg %zu len %zu forced %lld: %d passes", nseg, len, (long long)forced, p.passes);
  if (p.passes < 1 || p.passes > 32) return p;
  EXPECT(p.split[p.passes - 1] == 1, "nseg %zu len %zu: last split %u", nseg, len, p.split[p.passes - 1]);
  size_t cur = len;
  for (int k = 0; k < p.passes; ++k) {
    const size_t s = p.split[k];
    EXPECT(s >= 1 && s <= cur, "nseg %zu len %zu pass %d: split %zu of %zu", nseg, len, k, s, cur);
    if (s < 1 || s > cur) return p;
    if (k + 1 < p.passes) EXPECT(s > 1, "nseg %zu len %zu pass %d: split 1 before the end", nseg, len, k);
    if (k > 0 || forced < 1) EXPECT(s == 1 || 2 * s <= cur, "nseg %zu len %zu pass %d: planned split %zu of %zu", nseg, len, k, s, cur);
    if (cur <= 70000) walk_covers(cur, s);
    cur = s;
  }
  if (forced >= 1) EXPECT(p.split[0] == ((size_t)forced < len ? (size_t)forced : len), "forced %lld of %zu: %u", (long long)forced, len, p.split[0]);
  return p;
}

int main() {
  const size_t chip = 65536;
  const size_t lens[] = {1, 2, 3, 7, 8, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000, 4096, 5000, 65536, 65537, (size_t)1 << 20, ((size_t)1 << 20) + 1, (size_t)1 << 28};
  const size_t segs[] = {1, 2, 3, 65, 257, 4096, 65536, 65537, (size_t)1 << 20, (size_t)1 << 28};
  const int64_t forced[] = {-1, 0, 1, 2, 7, 64, 256, 1000, (int64_t)1 << 40};
  const int64_t runs[] = {8, 2, 1, 0, -5, 16, 1000};
  size_t n = 0;
  for (size_t len : lens)
    for (size_t nseg : segs) {
      if (len > (((size_t)1 << 28) / nseg)) continue;
      for (int64_t f : forced)
        for (int64_t r : runs) {
          check(nseg, len, f, r, chip);
          ++n;
        }
    }
  // what the defaults give for the shapes the rates are quoted for
  const struct { size_t nseg, len; } shapes[] = {{1, (size_t)1 << 20}, {4096, 256}, {65536, 16}, {1, 5000}, {257, 1}};
  for (auto s : shapes) {
    const SumPlan p = check(s.nseg, s.len, -1, 4, chip);
    printf("%zu x %zu:", s.nseg, s.len);
    for (int k = 0; k < p.passes; ++k) printf(" %u", p.split[k]);
    printf("\n");
  }
  {
    const SumPlan p = plan_sum(1, (size_t)1 << 20, chip, -1, 4);
    EXPECT(p.split[0] == 65536, "a lone segment of 2^20 fills the chip on its first pass: %u", p.split[0]);
    const SumPlan q = plan_sum(65536, 16, chip, -1, 4);
    EXPECT(q.passes == 1, "one lane per segment when the segments fill the chip: %d passes", q.passes);
    const SumPlan e = plan_sum(0, 5, chip, -1, 8);
    EXPECT(e.passes == 0, "nothing to plan: %d", e.passes);
  }
  printf("%zu configurations\n", n);
  if (fails) return 1;
  printf("ok\n");
  return 0;
}
