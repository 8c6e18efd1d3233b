// dispatch_test.cpp — the routing table of bgn_amd/csrc/dispatch.hpp, printed one configuration per line with its cases
// behind it (tests/test_dispatch_cpu.py builds it with the address and undefined-behaviour sanitizers and compares with
// tests/golden/dispatch_routes.txt; no GPU involved).
//
//   <nl> <table_walk> <option set> <work>: <count><L|C|Q: lane, cooperative, lane groups>[/<head, where not count>] ...
//   <nl> <option set> MultConst L<level>: k<scalar bytes>=<lane-group limit> ...
//
// Limb counts with the instantiations they really have (3: no lane groups; 72: no cooperative kernel), with and without
// the walk over the key's line table, under the defaults, every setting of the GPU tests' force helpers, the single
// options with a meaning of their own and one set of calibrated crossovers.  Counts: fixed ones around the lane
// kernel's rounds, and every threshold of the configuration with the count just above it.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "../../bgn_amd/csrc/dispatch.hpp"

using namespace bgn;

struct OptionSet {
  const char* name;
  std::vector<std::pair<Options::V Options::*, int64_t>> set;
  bool calibrated;
};

static std::vector<OptionSet> option_sets() {
  typedef Options O;
  const int64_t big = (int64_t)1 << 40, py = 100000000;
  std::vector<OptionSet> r;
  r.push_back({"defaults", {}, false});
  for (int k = 0; k < 3; ++k) {      // conftest.py EngineOptions.force: coop, quad, lane
    const int64_t c = k == 0 ? big : 0, q = k == 1 ? big : 0;
    r.push_back({k == 0 ? "force-coop" : k == 1 ? "force-quad" : "force-lane",
                 {{&O::quad_min, 0}, {&O::coop_max, c}, {&O::coop_max_l2, c}, {&O::coop_max_dec, c}, {&O::quad_max, q},
                  {&O::quad_max_l2, q}, {&O::quad_max_dec, q}, {&O::quad_max_pow, q}, {&O::quad_max_mc, q}},
                 false});
  }
  for (int k = 0; k < 3; ++k) {      // test_gpu_quad.py force
    r.push_back({k == 0 ? "pairs-coop" : k == 1 ? "pairs-quad" : "pairs-lane",
                 {{&O::quad_min, 0}, {&O::quad_max, k == 1 ? py : 0}, {&O::coop_max, k == 0 ? py : 0}}, false});
  }
  for (int k = 0; k < 3; ++k) {      // test_gpu_quad.py force_table
    const int64_t c = k == 0 ? py : 0, q = k == 1 ? py : 0;
    r.push_back({k == 0 ? "table-coop" : k == 1 ? "table-quad" : "table-lane",
                 {{&O::quad_min, 0}, {&O::quad_max_l2, q}, {&O::quad_max_dec, q}, {&O::quad_max_pow, q}, {&O::coop_max_l2, c},
                  {&O::coop_max_dec, c}},
                 false});
  }
  r.push_back({"coop_max=3000", {{&O::coop_max, 3000}}, false});            // alone: the historical A/B meaning
  r.push_back({"coop_max_l2=3000", {{&O::coop_max_l2, 3000}}, false});
  r.push_back({"coop_max_dec=3000", {{&O::coop_max_dec, 3000}}, false});
  r.push_back({"quad_min=100", {{&O::quad_min, 100}}, false});
  r.push_back({"quad_max_l2=20000,quad_min=0", {{&O::quad_max_l2, 20000}, {&O::quad_min, 0}}, false});
  r.push_back({"split_rounds=0", {{&O::split_rounds, 0}}, false});
  r.push_back({"calibrated", {}, true});
  return r;
}

int main() {
  struct Limbs { int nl; bool coop, quad, quad_mc; };
  const Limbs limbs[] = {{3, true, false, false}, {10, true, true, true}, {19, true, true, true},
                         {36, true, true, true},  {37, true, true, true}, {72, false, true, true}};
  const char* work_name[] = {"Mult", "MakeL2", "Lift", "Power"};
  const char family_name[] = {'L', 'C', 'Q'};
  const size_t fixed[] = {1, 65537, 70000, (size_t)1 << 20, ((size_t)1 << 20) + 1000, (size_t)1 << 22};
  const size_t klens[] = {1, 2, 3, 5, 15, 16, 128};
  for (const Limbs& l : limbs)
    for (const OptionSet& os : option_sets()) {
      Options opt;
      Crossovers xo;
      for (const auto& s : os.set) (opt.*(s.first)).store(s.second);
      if (os.calibrated) {
        const int64_t coop[4] = {900, 700, 1100, 1100}, quad[4] = {52000, 43000, 30000, 30000};
        for (int i = 0; i < 4; ++i) {
          xo.coop[i].store(coop[i]);
          xo.quad[i].store(quad[i]);
        }
      }
      for (int tw = 0; tw < 2; ++tw) {
        const DispatchView v{l.nl, tw != 0, l.coop, l.quad, l.quad_mc, &opt, &xo};
        for (int wi = 0; wi < 4; ++wi) {
          const Work w = (Work)wi;
          std::vector<size_t> counts(fixed, fixed + sizeof fixed / sizeof fixed[0]);
          for (size_t t : {detail::coop_limit(v, w), detail::quad_floor(v, w), detail::quad_max(v, w)})
            for (size_t c : {t, t + 1})
              if (c >= 1 && c <= kMaxBatch) counts.push_back(c);
          std::sort(counts.begin(), counts.end());
          counts.erase(std::unique(counts.begin(), counts.end()), counts.end());
          printf("%d %d %s %s:", l.nl, tw, os.name, work_name[wi]);
          for (size_t n : counts) {
            printf(" %zu%c", n, family_name[(int)family(v, w, n)]);
            if (rounds_head(v, w, n) != n) printf("/%zu", rounds_head(v, w, n));
          }
          printf("\n");
        }
        if (tw) continue;      // MultConst's limit does not read the table walk
        for (int level = 1; level <= 2; ++level) {
          printf("%d %s MultConst L%d:", l.nl, os.name, level);
          for (size_t k : klens) printf(" k%zu=%zu", k, multconst_quad_limit(v, level, k));
          printf("\n");
        }
      }
    }
  return 0;
}
