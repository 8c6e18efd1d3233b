// group_plan_test.cpp — the column groups of bgn_lincomb_batch without a GPU: the balanced-ternary codes and the table's
// recurrence of grprecode.hpp over plain integers, and the properties of dispatch.hpp plan_lincomb_groups / lin_path.
// Prints "ok", or the violated property and exits 1.  Built by tests/test_group_plan_cpu.py with the address and UB
// sanitizers.
#include <cstdio>
#include <vector>

#include "../../bgn_amd/csrc/dispatch.hpp"
#include "../../bgn_amd/csrc/grprecode.hpp"

using namespace bgn;

static int fails = 0;
#define EXPECT(cond, ...) \
  do { if (!(cond)) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); ++fails; } } while (0)

// Every trit vector of a group of g: its code round-trips, and the recurrence over the integers x_i reproduces sum tau_i x_i.
static void codes_and_recurrence(int g) {
  const int M = grp_entries(g), n3 = grp_pow3(g);
  EXPECT(M == (n3 - 1) / 2 && M <= 32767 && (size_t)M == grp_plan_entries(g), "g %d", g);
  const long x[kGrpMaxGroup] = {1000003, -77, 5, 123456789, -31, 999};
  std::vector<long> entry(M + 1, 0);
  std::vector<char> done(M + 1, 0);
  for (int k = 0; k < g; ++k)
    for (int j = 0; j < grp_pow3(k); ++j) {
      const int cp = grp_level_rest(k, j), c = grp_level_entry(k, j), a = cp < 0 ? -cp : cp;
      EXPECT(c >= 1 && c <= M && !done[c] && c - cp == grp_pow3(k), "g %d level %d entry %d", g, k, c);
      EXPECT(a <= (grp_pow3(k) - 1) / 2 && (a == 0 || done[a]), "g %d entry %d reads %d", g, c, a);      // lower levels only
      entry[c] = x[k] + (cp < 0 ? -entry[a] : entry[a]);
      done[c] = 1;
    }
  for (int c = 1; c <= M; ++c) EXPECT(done[c], "g %d entry %d never built", g, c);
  for (int v = 0; v < n3; ++v) {                        // all of {-1, 0, 1}^g
    int32_t w[kGrpMaxGroup];
    int tau[kGrpMaxGroup], back[kGrpMaxGroup];
    long sum = 0;
    for (int i = 0, r = v; i < g; ++i, r /= 3) {
      tau[i] = r % 3 - 1;
      w[i] = tau[i] * 3;                               // m = 3 at w_bits = 2: the trit on both planes
      sum += tau[i] * x[i];
    }
    int16_t code[kGrpMaxBits];
    grp_codes(w, g, 2, code);
    EXPECT(code[0] == code[1] && code[0] >= -M && code[0] <= M, "g %d vector %d", g, v);
    grp_trits(code[0], g, back);
    for (int i = 0; i < g; ++i) EXPECT(back[i] == tau[i], "g %d vector %d trit %d", g, v, i);
    const int c = code[0];
    EXPECT((c == 0 ? 0 : c < 0 ? -entry[-c] : entry[c]) == sum, "g %d vector %d", g, v);
  }
  // a ragged group (fewer weights than g) has zero trits above; a weight counts reduced, with its sign
  const int32_t w2[2] = {-(16 + 5), 6};
  int16_t code[kGrpMaxBits];
  grp_codes(w2, 2, 4, code);
  EXPECT(code[0] == -1 && code[1] == 3 && code[2] == -1 + 3 && code[3] == 0, "planes of (-5, 6)");
}

static const size_t kBudget = (size_t)64 << 30;

static void planner() {
  const size_t shapes[][3] = {{1, 1, 1}, {1, 65, 4}, {2, 3, 6}, {1, 65, 33}, {1, 4096, 4096}, {64, 16, 256}, {1, 1, (size_t)1 << 20},
                              {1, 16, 1024}, {1, (size_t)1 << 14, (size_t)1 << 14}, {1, 1, (size_t)1 << 28}};
  for (const auto& sh : shapes)
    for (int level = 1; level <= 2; ++level)
      for (int w_bits : {1, 2, 4, 5, 9, 31})
        for (int64_t groups : {-1, 0, 1, 2, 5, 6, 99})
          for (size_t budget : {kBudget, (size_t)1 << 20})
            for (int64_t split : {-1, 1, 3, 1000000}) {
              const size_t nvec = sh[0], nrows = sh[1], d = sh[2], eb = level == 1 ? 577 : 288;
              const GrpPlan p = plan_lincomb_groups(nvec, nrows, d, w_bits, budget, eb, level, 65536, -1, split, groups);
              const LinPlan t = plan_lincomb(nvec, nrows, d, w_bits, budget, eb, level, 65536, -1, split);
#define WHERE "%zu x %zu x %zu w_bits %d level %d groups %lld budget %zu split %lld", nvec, nrows, d, w_bits, level, (long long)groups, budget, (long long)split
              EXPECT(p.table.omega == t.omega && p.table.nwin == t.nwin && p.table.nchunk == t.nchunk && p.table.entries == t.entries, WHERE);
              if (groups == 0 || w_bits > 4) EXPECT(!p.use, WHERE);
              if (!p.use) continue;
              EXPECT(p.g >= 2 && p.g <= 6 && p.M == grp_plan_entries(p.g) && p.ngroups == (d + p.g - 1) / p.g, WHERE);
              EXPECT(p.entries == nvec * p.ngroups * p.M && p.entries <= kMaxBatch && p.entries <= budget / eb, WHERE);
              EXPECT(p.nchunk >= 1 && p.nchunk <= p.ngroups && nvec * nrows * p.nchunk <= kMaxBatch, WHERE);
              if (groups > 0) EXPECT(p.g <= (groups < 2 ? 2 : groups > 6 ? 6 : (int)groups), WHERE);
              if (groups < 0) EXPECT(nrows >= kGrpMinRows && d >= kGrpMinCols && p.cost < p.table_cost, WHERE);
              if (split >= 1) EXPECT(p.nchunk == ((size_t)split < p.ngroups ? (size_t)split : p.ngroups), WHERE);
            }
  // narrowed rather than refused: 2^22 columns at g = 5 are 10^8 entries, over a 16 GB budget on level 1; g = 2 fits
  const GrpPlan n = plan_lincomb_groups(1, 4096, (size_t)1 << 22, 1, (size_t)16 << 30, 577, 1, 65536, -1, -1, 5);
  EXPECT(n.use && n.g >= 2 && n.g < 5 && n.entries <= ((size_t)16 << 30) / 577, "narrowed to %d", n.g);
  const GrpPlan f = plan_lincomb_groups(1, 4096, 4096, 1, kBudget, 577, 1, 65536, -1, -1, 5);
  EXPECT(f.use && f.g == 5 && f.ngroups == 820 && f.M == 121, "forced 5");
  EXPECT(!plan_lincomb_groups(1, 4096, (size_t)1 << 22, 1, 1000, 577, 1, 65536, -1, -1, 5).use, "nothing fits");
  // precedence
  BktPlan b0, b1;
  b1.use = true;
  GrpPlan g0, g1;
  g1.use = true;
  EXPECT(lin_path(b1, g1, 1, 5) == LinPath::Buckets, "forced buckets win over everything");
  EXPECT(lin_path(b1, g1, -1, 5) == LinPath::Groups, "a forced group size wins over planned buckets");
  EXPECT(lin_path(b1, g1, -1, -1) == LinPath::Buckets, "planned buckets win over planned groups");
  EXPECT(lin_path(b0, g1, -1, -1) == LinPath::Groups && lin_path(b0, g1, 0, 2) == LinPath::Groups, "groups");
  EXPECT(lin_path(b0, g0, -1, -1) == LinPath::Tables && lin_path(b0, g0, 1, 5) == LinPath::Tables, "tables");
  // planned where it measured a gain; the long single row stays where it is
  EXPECT(plan_lincomb_groups(1, 4096, 4096, 1, kBudget, 577, 1, 65536, -1, -1, -1).use, "1 x 4096 x 4096");
  EXPECT(!plan_lincomb_groups(1, 1024, 1024, 1, kBudget, 577, 1, 65536, -1, -1, -1).use, "1 x 1024 x 1024");
  EXPECT(!plan_lincomb_groups(1, 1, (size_t)1 << 20, 1, kBudget, 577, 1, 65536, -1, -1, -1).use, "1 x 1 x 2^20");
}

int main() {
  for (int g = 2; g <= kGrpMaxGroup; ++g) codes_and_recurrence(g);
  static_assert(kGrpPlanMaxBits == kGrpMaxBits && kGrpPlanMaxGroup == kGrpMaxGroup, "dispatch.hpp restates grprecode.hpp");
  planner();
  if (fails) return 1;
  printf("ok\n");
  return 0;
}
