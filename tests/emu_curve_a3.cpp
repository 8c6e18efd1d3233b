// emu_curve_a3.cpp — host emulation of Mult's Miller loop on the a = -3 curve (TEST INFRASTRUCTURE, built by
// tests/test_emu_curve_a3.py the way tests/emu/emu.py builds emu.cpp): the key constant of hostbig.hpp, the decode
// with per-coordinate factors, and the step programs of pairing.hpp with PairOperands::a3 set, range checks on.
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>

thread_local int bgn_emu_checks = 0;
thread_local unsigned long long bgn_emu_tally[16] = {0};
struct EmuChecks { EmuChecks() { bgn_emu_checks = 1; } ~EmuChecks() { bgn_emu_checks = 0; } };
thread_local EmuDim3 threadIdx = {0, 0, 0}, blockIdx = {0, 0, 0}, gridDim = {1, 1, 1}, blockDim = {256, 1, 1};

#include "ops.hpp"
#include "codec.hpp"
#include "fpinv.hpp"
#include "hostbig.hpp"

using namespace bgn;

template <int NL>
struct A3 {
  static LFp<NL>* lds() {
    static LFp<NL> L[4];
    return L;
  }
  // what k_decode does with factor pointers: wire -> (fx*x/R, fy*y/R), canonical
  static void decode(const u32* params, const uint8_t* wire, int Lb, const u32* fx, const u32* fy, u32* out) {
    EmuChecks on;
    const FpParams<NL>* P = (const FpParams<NL>*)params;
    Fp<NL> x, y, m;
    wire_to_limbs<NL>(x, wire, Lb);
    wire_to_limbs<NL>(y, wire + Lb, Lb);
    fp_to_mont_scaled<NL>(m, x, fx ? fx : P->r2, P, lds());
    memcpy(out, m.v, 4 * NL);
    fp_to_mont_scaled<NL>(m, y, fy ? fy : P->r2, P, lds());
    memcpy(out + NL, m.v, 4 * NL);
  }
  // one pairing as a lane of k_pairing<NL, 0> with run == 1 computes it: the windowed loop or the plain NAF
  static void pairing(const u32* params, const PairingConsts* C, const u32* a, const u32* b, int a3, int windowed, u32* out) {
    EmuChecks on;
    const FpParams<NL>* P = (const FpParams<NL>*)params;
    LFp<NL>* L = lds();
    PairOperands op{a, a + NL, 1, 0, b, b + NL, 1, 0};
    op.a3 = a3;
    std::vector<u32> win((size_t)WIN_SLOTS * NL);
    WinTab W{win.data(), 1, 0};
    Miller<NL> S;
    if (windowed)
      miller_loop_w<NL>(S, L, op, W, C, P);
    else
      miller_loop<NL>(S, L, op, C, P);
    Fp<NL> N, ninv, g0, g1, re, im;
    miller_norm<NL>(N, S, L, P);
    fp_inv_mont<NL>(ninv, N, C->pm2_bits + 1, P, L);
    final_exp_with_inverse<NL>(g0, g1, S, ninv, L, C, P);
    fp_from_mont<NL>(im, g1, P, L);
    fp_from_mont<NL>(re, g0, P, L);
    memcpy(out, re.v, 4 * NL);
    memcpy(out + NL, im.v, 4 * NL);
  }
  // doubling, doubling, addition, doubling from a GIVEN state (x, y, z, f0, f1: raw limbs at the bounds the step
  // programs document) with operands a, b (canonical): only the range checks matter, the values are arbitrary
  static void steps(const u32* params, const u32* st, const u32* a, const u32* b, int a3, u32* out) {
    EmuChecks on;
    const FpParams<NL>* P = (const FpParams<NL>*)params;
    LFp<NL>* L = lds();
    PairOperands op{a, a + NL, 1, 0, b, b + NL, 1, 0};
    op.a3 = a3;
    Miller<NL> S;
    Fp<NL> r;
    AFp<NL>* slot[5] = {&S.X, &S.Y, &S.Z, &S.F0, &S.F1};
    for (int k = 0; k < 5; ++k) {
      memcpy(r.v, st + (size_t)k * NL, 4 * NL);
      a_store(*slot[k], r);
    }
    miller_double<NL>(S, L, op, P);
    miller_double<NL>(S, L, op, P);
    miller_add<NL>(S, L, op, 1, P);
    miller_double<NL>(S, L, op, P);
    miller_add<NL>(S, L, op, -1, P);
    miller_double<NL>(S, L, op, P);
    for (int k = 0; k < 5; ++k) {
      a_load(r, *slot[k]);
      memcpy(out + (size_t)k * NL, r.v, 4 * NL);
    }
  }
};

#define DISPATCH(nl, call)            \
  switch (nl) {                       \
    case 3: A3<3>::call; break;       \
    case 10: A3<10>::call; break;     \
    case 19: A3<19>::call; break;     \
    case 36: A3<36>::call; break;     \
    case 37: A3<37>::call; break;     \
    default: return -1;               \
  }                                   \
  return 0;

extern "C" {
int a3_decode(int nl, const u32* params, const uint8_t* wire, int Lb, const u32* fx, const u32* fy, u32* out) { DISPATCH(nl, decode(params, wire, Lb, fx, fy, out)) }
int a3_pairing(int nl, const u32* params, const void* C, const u32* a, const u32* b, int a3, int windowed, u32* out) { DISPATCH(nl, pairing(params, (const PairingConsts*)C, a, b, a3, windowed, out)) }
int a3_steps(int nl, const u32* params, const u32* st, const u32* a, const u32* b, int a3, u32* out) { DISPATCH(nl, steps(params, st, a, b, a3, out)) }
// hostbig.hpp curve_a3_root: 1 and u (big-endian, p_len bytes) when p has a fourth root of -3, else 0
int a3_root(const uint8_t* p_be, size_t p_len, uint8_t* u_be) {
  BigU u;
  if (!curve_a3_root(BigU::from_be(p_be, p_len), u)) return 0;
  memset(u_be, 0, p_len);
  for (size_t i = 0; i < p_len && i / 4 < u.w.size(); ++i) u_be[p_len - 1 - i] = (uint8_t)(u.w[i / 4] >> (8 * (i % 4)));
  return 1;
}
}
