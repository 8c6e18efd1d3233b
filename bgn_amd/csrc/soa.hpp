// soa.hpp — the structure-of-arrays view that the kernels and the host's workspace planner (carve.hpp) share.
// Free of HIP, so that carve.hpp builds without it.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bgn {

// Device-side SoA view of `count` F_p^2-sized elements (a G1 point x,y or a GT
// element re,im): limb j of element e at c0[j*stride + e].
struct SoA2 {
  uint32_t* c0;
  uint32_t* c1;
  uint8_t* inf;     // per-element identity flag (G1 only; may be null for GT)
  size_t stride;
};

}  // namespace bgn
