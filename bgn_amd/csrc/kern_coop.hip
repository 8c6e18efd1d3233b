// kern_coop.hip — instantiations of the wave-cooperative pairing kernel for every limb count.
#include "coop/coop.hpp"
#include "coop/coop_api.hpp"

namespace bgn {

size_t coop_ws_words(int nl, size_t sw) { return (size_t)COOP_PARK_WORDS * sw + (size_t)2 * nl * sw; }

template <int NL>
static void launch(hipStream_t s, const void* params, int p_bits, const PairingJob& j) {
  const FpParams<NL>* P = (const FpParams<NL>*)params;
  const size_t count = j.count, sw = j.sw;
  const int shape = (int)j.shape;
  const dim3 grid((unsigned)count), block(COOP_BLOCK);
  if (!j.ws) {
    hipLaunchKernelGGL((k_pairing_coop<NL>), grid, block, 0, s, P, j.consts, j.a, j.b, j.out, count, shape, j.d1, j.d2, 0, nullptr,
                       nullptr, nullptr, (size_t)0, j.tab);
    return;
  }
  uint32_t* park = j.ws;
  uint32_t* nsoa = j.ws + (size_t)COOP_PARK_WORDS * sw;
  uint32_t* isoa = nsoa + (size_t)NL * sw;
  hipLaunchKernelGGL((k_pairing_coop<NL>), grid, block, 0, s, P, j.consts, j.a, j.b, j.out, count, shape, j.d1, j.d2, 1, park, nsoa,
                     isoa, sw, j.tab);
  hipLaunchKernelGGL((k_coop_invert<NL>), dim3((unsigned)((count + FP_BLOCK - 1) / FP_BLOCK)), dim3(FP_BLOCK), 0, s, P, nsoa,
                     isoa, sw, count, p_bits);
  hipLaunchKernelGGL((k_pairing_coop<NL>), grid, block, 0, s, P, j.consts, j.a, j.b, j.out, count, shape, j.d1, j.d2, 2, park, nsoa,
                     isoa, sw, j.tab);
}

bool coop_pairing_launch(int nl, hipStream_t s, const void* params, int p_bits, const PairingJob& job) {
  if (!job.count) return true;
  switch (nl) {
    case 3: launch<3>(s, params, p_bits, job); return true;
    case 10: launch<10>(s, params, p_bits, job); return true;
    case 19: launch<19>(s, params, p_bits, job); return true;
    case 36: launch<36>(s, params, p_bits, job); return true;
    case 37: launch<37>(s, params, p_bits, job); return true;
  }
  return false;
}

template <int NL>
static void launch_pow(hipStream_t s, const void* params, const uint32_t* a0, const uint32_t* a1, size_t sa, const uint8_t* k,
                       size_t kstride, size_t klen, uint32_t* o0, uint32_t* o1, size_t so, size_t count) {
  hipLaunchKernelGGL((k_gt_pow_coop<NL>), dim3((unsigned)count), dim3(COOP_BLOCK), 0, s, (const FpParams<NL>*)params, a0, a1,
                     sa, k, kstride, klen, o0, o1, so, count);
}

bool coop_gt_pow_launch(int nl, hipStream_t s, const void* params, const uint32_t* a0, const uint32_t* a1, size_t sa,
                        const uint8_t* k, size_t kstride, size_t klen, uint32_t* o0, uint32_t* o1, size_t so, size_t count) {
  if (!count) return true;
  if (klen > 256) return false;
  switch (nl) {
    case 3: launch_pow<3>(s, params, a0, a1, sa, k, kstride, klen, o0, o1, so, count); return true;
    case 10: launch_pow<10>(s, params, a0, a1, sa, k, kstride, klen, o0, o1, so, count); return true;
    case 19: launch_pow<19>(s, params, a0, a1, sa, k, kstride, klen, o0, o1, so, count); return true;
    case 36: launch_pow<36>(s, params, a0, a1, sa, k, kstride, klen, o0, o1, so, count); return true;
    case 37: launch_pow<37>(s, params, a0, a1, sa, k, kstride, klen, o0, o1, so, count); return true;
  }
  return false;
}

// ---- field arithmetic on its own (bgn_field_ops_family_batch: the parity tests' direct view of coop_mul, coop_operand,
// coop_combo, coop_normalize and coop_canonical; diagnostics, no operation runs on it) ---------------------------------
// One element per wave.  xy: canonical Montgomery SoA (x in c0, y in c1); prod = (x*y, (x-y)*(x+y)), sqr = (x^2, y^2),
// lin = (x+y, x-y), plain canonical SoA.  Every value is handled as the interpreter handles it: a product's operands
// come from the wave's slots through coop_operand — x*y and the squares in the plain-stored form, x - y (+ p: y is
// below p, the generator's choice of the multiple) and x + y as two-term sums —, a result is stored through
// coop_normalize, the sums of `lin` are linear micro-ops, and a value leaves Montgomery form by a product with the raw
// 1 before coop_canonical.  Nothing of fpmont.hpp is called.
constexpr int COOP_FIELD_WAVES = 4;                 // elements per workgroup
enum { COOP_FIELD_X = 0, COOP_FIELD_Y = 1, COOP_FIELD_RAW1 = 2, COOP_FIELD_T = 3, COOP_FIELD_NSLOTS = 4 };

template <int NL>
__global__ void __launch_bounds__(64 * COOP_FIELD_WAVES)
k_field_ops_coop(const FpParams<NL>* __restrict__ P, SoA2 xy, SoA2 prod, SoA2 sqr, SoA2 lin, size_t count) {
  __shared__ u32 Vs[COOP_FIELD_WAVES][COOP_FIELD_NSLOTS][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const size_t e = (size_t)blockIdx.x * COOP_FIELD_WAVES + (size_t)wave;
  if (e >= count) return;                           // a whole wave: no barrier follows, a wave reads only its own slots
  u32 (*V)[64] = Vs[wave];
  CoopLane<NL> c;
  c.lane = lane;
  c.p = lane < NL ? P->p[lane < NL ? lane : 0] : 0u;
  c.keep = lane < NL - 1 ? LIMB_MASK : 0xFFFFFFFFu;
  c.carry = lane < NL - 1 ? 0xFFFFFFFFu : 0u;
  c.pinv = P->pinv;
  const int lj = lane < NL ? lane : 0;
  const bool in = lane < NL;
  V[COOP_FIELD_X][lane] = in ? xy.c0[(size_t)lj * xy.stride + e] : 0u;
  V[COOP_FIELD_Y][lane] = in ? xy.c1[(size_t)lj * xy.stride + e] : 0u;
  V[COOP_FIELD_RAW1][lane] = lane == 0 ? 1u : 0u;
  constexpr u32 XY = (u32)COOP_FIELD_X | (u32)COOP_FIELD_Y << 8;
  constexpr u32 PLUS = 0x0101u, MINUS = 0xFF01u;    // coefficients (1, 1) and (1, -1), a byte each
  // t: a stored value below 2p in Montgomery form -> its canonical plain residue
  auto leave = [&](u32 t, u32* dst, size_t stride) {
    V[COOP_FIELD_T][lane] = t;
    const u32 a = coop_operand<NL>(V, true, (u32)COOP_FIELD_T, 0u, 0, c);
    const u32 b = coop_operand<NL>(V, true, (u32)COOP_FIELD_RAW1, 0u, 0, c);
    const u32 r = coop_canonical<NL>(coop_normalize<NL>((long long)coop_mul<NL>(a, b, c), c), c);
    if (in) dst[(size_t)lj * stride + e] = r;
  };
  auto product = [&](u32 a, u32 b) { return coop_normalize<NL>((long long)coop_mul<NL>(a, b, c), c); };
  const u32 x = coop_operand<NL>(V, true, (u32)COOP_FIELD_X, 0u, 0, c);
  const u32 y = coop_operand<NL>(V, true, (u32)COOP_FIELD_Y, 0u, 0, c);
  leave(product(x, y), prod.c0, prod.stride);
  leave(product(coop_operand<NL>(V, false, XY, MINUS, 1, c), coop_operand<NL>(V, false, XY, PLUS, 0, c)), prod.c1, prod.stride);
  leave(product(x, x), sqr.c0, sqr.stride);
  leave(product(y, y), sqr.c1, sqr.stride);
  leave(coop_normalize<NL>(coop_combo<NL>(V, 2, XY, PLUS, 0, c), c), lin.c0, lin.stride);
  leave(coop_normalize<NL>(coop_combo<NL>(V, 2, XY, MINUS, 1, c), c), lin.c1, lin.stride);
}

template <int NL>
static void launch_field(hipStream_t s, const void* params, SoA2 xy, SoA2 prod, SoA2 sqr, SoA2 lin, size_t count) {
  hipLaunchKernelGGL((k_field_ops_coop<NL>), dim3((unsigned)((count + COOP_FIELD_WAVES - 1) / COOP_FIELD_WAVES)),
                     dim3(64 * COOP_FIELD_WAVES), 0, s, (const FpParams<NL>*)params, xy, prod, sqr, lin, count);
}

bool coop_field_ops_launch(int nl, hipStream_t s, const void* params, SoA2 xy, SoA2 prod, SoA2 sqr, SoA2 lin, size_t count) {
  switch (nl) {
    case 3: if (count) launch_field<3>(s, params, xy, prod, sqr, lin, count); return true;
    case 10: if (count) launch_field<10>(s, params, xy, prod, sqr, lin, count); return true;
    case 19: if (count) launch_field<19>(s, params, xy, prod, sqr, lin, count); return true;
    case 36: if (count) launch_field<36>(s, params, xy, prod, sqr, lin, count); return true;
    case 37: if (count) launch_field<37>(s, params, xy, prod, sqr, lin, count); return true;
  }
  return false;
}

const char* coop_pairing_kernel_name(int nl) {
  switch (nl) {
    case 3: return "k_pairing_coop<3>";
    case 10: return "k_pairing_coop<10>";
    case 19: return "k_pairing_coop<19>";
    case 36: return "k_pairing_coop<36>";
    case 37: return "k_pairing_coop<37>";
  }
  return "";
}

}  // namespace bgn
