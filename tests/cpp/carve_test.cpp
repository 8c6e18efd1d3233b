// carve_test.cpp — the workspace planner of bgn_amd/csrc/carve.hpp on the CPU (tests/test_carve_cpu.py builds it with
// the address and undefined-behaviour sanitizers).  A stub context whose arena is a heap block of exactly the size the
// sizing pass asked for: the carving pass must end at that size, every array must be 256-byte aligned inside the
// block and apart from the others (each is filled, so the sanitizer sees any byte outside the block), and the
// offsets must be the ones worked out here by hand from "every take is rounded up to 256 bytes".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct Ctx {
  int nl;
  uint8_t* arena = nullptr;
  size_t arena_bytes = 0;
  int fail_with = 0;
};
int ensure_arena(Ctx* c, size_t bytes) {
  if (c->fail_with) return c->fail_with;
  free(c->arena);
  c->arena = (uint8_t*)aligned_alloc(256, bytes);      // (every size asked for is a multiple of 256)
  c->arena_bytes = bytes;
  return 0;
}

#include "../../bgn_amd/csrc/carve.hpp"

using namespace bgn;

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      fprintf(stderr, "%s:%d: %s (nl %d, stride %zu, gt %d)\n", __FILE__, __LINE__, #cond, nl, st, (int)with_gt); \
      exit(1);                                                           \
    }                                                                    \
  } while (0)

static size_t r256(size_t v) { return (v + 255) / 256 * 256; }

static void run(int nl, size_t st, bool with_gt) {
  Ctx c;
  c.nl = nl;
  SoA2 A{}, X{};
  uint32_t* row = nullptr;
  uint8_t *one = nullptr, *odd = nullptr;
  int passes = 0;
  auto layout = [&](Ws& w) {
    ++passes;
    A = w.g1(st);
    if (with_gt) X = w.gt(st);
    row = w.fp(st);
    one = (uint8_t*)w.cv.take(1);
    odd = (uint8_t*)w.cv.take(257);
  };
  CHECK(carve(&c, layout) == 0 && passes == 2);
  // by hand: limb arrays of nl * st u32, identity flags of st bytes
  const size_t limb = r256((size_t)nl * st * 4);
  struct Region { const void* p; size_t off, bytes; };
  std::vector<Region> want;
  size_t off = 0;
  auto add = [&](const void* p, size_t bytes, size_t rounded) {
    want.push_back({p, off, bytes});
    off += rounded;
  };
  add(A.c0, (size_t)nl * st * 4, limb);
  add(A.c1, (size_t)nl * st * 4, limb);
  add(A.inf, st, r256(st));
  if (with_gt) {
    add(X.c0, (size_t)nl * st * 4, limb);
    add(X.c1, (size_t)nl * st * 4, limb);
  }
  add(row, (size_t)nl * st * 4, limb);
  add(one, 1, 256);
  add(odd, 257, 512);
  CHECK(A.stride == st && (!with_gt || (X.stride == st && X.inf == nullptr)));
  CHECK(c.arena_bytes == off);                                   // 1. the sizing pass reports the carving pass's end
  for (size_t i = 0; i < want.size(); ++i) {
    const uint8_t* p = (const uint8_t*)want[i].p;
    CHECK(p == c.arena + want[i].off);                           // 3. the offsets worked out by hand
    CHECK(((uintptr_t)p & 255) == 0 && p >= c.arena && p + want[i].bytes <= c.arena + c.arena_bytes);      // 2.
    for (size_t k = 0; k < i; ++k) {
      const uint8_t* q = (const uint8_t*)want[k].p;
      CHECK(p + want[i].bytes <= q || q + want[k].bytes <= p);
    }
    memset((void*)p, (int)i + 1, want[i].bytes);
  }
  for (size_t i = 0; i < want.size(); ++i) {                     // no fill reached another array
    const uint8_t* p = (const uint8_t*)want[i].p;
    CHECK(p[0] == i + 1 && p[want[i].bytes - 1] == i + 1);
  }
  // an arena that cannot grow: the error comes back and nothing is carved
  c.fail_with = 7;
  passes = 0;
  CHECK(carve(&c, layout) == 7 && passes == 1 && A.c0 == nullptr && odd == nullptr);
  free(c.arena);
}

int main() {
  int n = 0;
  for (int nl : {3, 36})
    for (size_t st : {(size_t)64, (size_t)128})
      for (bool with_gt : {false, true}) {
        run(nl, st, with_gt);
        ++n;
      }
  printf("ok %d\n", n);
  return 0;
}
