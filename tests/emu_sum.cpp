// emu_sum.cpp — host emulation of one reduction pass of the segmented sums (TEST INFRASTRUCTURE, built by
// tests/test_emu_sum.py the way tests/test_emu_randexp.py builds its library): the geometry of csrc/sumops.hpp
// (sum_lane, sum_run_len: which elements lane (s, t) walks) and its lane functions — the Barrett accumulator of level 2,
// the Montgomery one, the Jacobian accumulator of level 1 with its conversion — one lane after the other, from wire
// bytes to wire bytes through the byte codec.  The staging through LDS is not emulated.
#include <hip/hip_runtime.h>
#include <string.h>

thread_local int bgn_emu_checks = 0;
thread_local unsigned long long bgn_emu_tally[16] = {0};
thread_local EmuDim3 threadIdx = {0, 0, 0}, blockIdx = {0, 0, 0}, gridDim = {1, 1, 1}, blockDim = {256, 1, 1};

#include "sumops.hpp"

using namespace bgn;

// mode 1: level 1; mode 2: level 2, Barrett; mode 3: level 2, Montgomery
template <int NL>
static void pass(const u32* params, const u32* mu, int pm2_bits, int mode, const uint8_t* in, int L, size_t nseg, u32 len,
                 u32 split, uint8_t* out) {
  static LFp<NL> Ls[4];
  static PairingConsts C;
  static BarrettParams<NL> Bp;
  static u32 sc[NL];
  const FpParams<NL>* P = (const FpParams<NL>*)params;
  memset(&C, 0, sizeof C);
  C.pm2_bits = pm2_bits;
  memset(&Bp, 0, sizeof Bp);
  for (int k = 0; k < NL + 2; ++k) Bp.mu[k] = mu[k];
  const size_t EB = (size_t)(2 * L);
  const size_t blocks = sum_blocks(nseg, split);
  const u32 steps = sum_steps(len, split);
  for (size_t b = 0; b < blocks; ++b)
    for (u32 tid = 0; tid < (u32)FP_BLOCK; ++tid) {
      threadIdx.x = tid;
      const SumLane ln = sum_lane(b, tid, nseg, split);
      if (!ln.ok) continue;
      Fp<NL> acc0, acc1;
      fp_zero(acc0);
      fp_zero(acc1);
      acc0.v[0] = 1;
      JacAcc<NL> S;
      bool acc_inf = true;
      if (mode == 1) sum_g1_init<NL>(S, acc_inf, P);
      if (mode == 3) sum_gt_mont_init<NL>(S.X, S.Y, P);
      for (u32 j = 0; j < steps; ++j) {
        const u32 n = sum_run_len(ln, j, len, split);
        if (!n) break;
        const bool live = ln.t - ln.t0 < n;
        // an idle lane decodes the first element of its workgroup's slice, as the kernel does
        const size_t e = (live ? ln.seg : ln.seg0) * (size_t)len + (size_t)j * split + (live ? ln.t : ln.t0);
        Fp<NL> x, y;
        wire_to_limbs<NL>(x, in + e * EB, L);
        wire_to_limbs<NL>(y, in + e * EB + L, L);
        if (mode == 1) {
          sum_g1_step<NL>(S, acc_inf, x, y, live, Ls, P);
        } else if (mode == 2) {
          sum_gt_take<NL>(x, y, live, P, &Bp);
          if (j == 0) {
            acc0 = x;
            acc1 = y;
          } else {
            sum_gt_step<NL>(acc0, acc1, x, y, P, &Bp, sc, 1);
          }
        } else {
          sum_gt_mont_step<NL>(S.X, S.Y, x, y, live, Ls, P);
        }
      }
      if (mode == 1) sum_g1_finish<NL>(acc0, acc1, S, acc_inf, Ls, &C, P);
      if (mode == 3) sum_gt_mont_finish<NL>(acc0, acc1, S.X, S.Y, Ls, P);
      uint8_t* dst = out + (ln.seg * (size_t)split + ln.t) * EB;
      limbs_to_wire<NL>(dst, L, acc0);
      limbs_to_wire<NL>(dst + L, L, acc1);
    }
}

#define EACH_NL(X) X(3) X(10) X(19) X(36) X(37)

extern "C" {
int sum_emu_block() { return FP_BLOCK; }

// nseg x len wire elements of `in` -> nseg x split wire elements of `out` (split <= len); -1: unknown limb count
int sum_emu_pass(int nl, const u32* params, const u32* mu, int pm2_bits, int mode, const uint8_t* in, int L,
                 unsigned long long nseg, unsigned len, unsigned split, uint8_t* out) {
  if (mode < 1 || mode > 3 || !split || split > len) return -2;
  switch (nl) {
#define X(N) case N: pass<N>(params, mu, pm2_bits, mode, in, L, (size_t)nseg, len, split, out); break;
    EACH_NL(X)
#undef X
    default: return -1;
  }
  return 0;
}
}
