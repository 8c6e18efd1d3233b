// carve.hpp — the workspace planner of engine.cpp: arrays carved out of one device allocation, every take rounded up
// to 256 bytes.  Host only and free of HIP (tests/cpp/carve_test.cpp runs it without a GPU).  The including file
// declares, before this header, `int ensure_arena(Ctx*, size_t bytes)` for its context type: it makes c->arena hold at
// least `bytes` and returns 0, or an error code.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "soa.hpp"

namespace bgn {

// Carves SoA2 views out of `base`; against a null base it only adds up the sizes.
struct Carver {
  uint8_t* base;
  size_t off = 0;
  explicit Carver(uint8_t* b) : base(b) {}
  void* take(size_t bytes) {
    void* p = base ? base + off : nullptr;
    off += (bytes + 255) / 256 * 256;
    return p;
  }
  SoA2 soa(int nl, size_t stride, bool with_inf) {
    SoA2 s;
    s.c0 = (uint32_t*)take((size_t)nl * stride * 4);
    s.c1 = (uint32_t*)take((size_t)nl * stride * 4);
    s.inf = with_inf ? (uint8_t*)take(stride) : nullptr;
    s.stride = stride;
    return s;
  }
};

struct Ws {   // the arrays of one call, by kind, for a field of nl limbs
  int nl;
  Carver cv;
  Ws(int nl_, uint8_t* base) : nl(nl_), cv(base) {}
  SoA2 g1(size_t stride) { return cv.soa(nl, stride, true); }
  SoA2 gt(size_t stride) { return cv.soa(nl, stride, false); }
  uint32_t* fp(size_t stride) { return (uint32_t*)cv.take((size_t)nl * stride * 4); }};

// layout(Ws&) runs twice: against null to size, then, after ensure_arena, against the arena.  It must take the same
// arrays in the same order both times (conditions on anything but the pointers it is handed are fine).
template <class Ctx, class F>
int carve(Ctx* c, F&& layout) {
  Ws probe(c->nl, nullptr);
  layout(probe);
  if (int rc = ensure_arena(c, probe.cv.off)) return rc;
  Ws w(c->nl, c->arena);
  layout(w);
  return 0;
}

}  // namespace bgn
