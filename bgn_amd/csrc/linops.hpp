// linops.hpp — linear maps of ciphertext vectors with plaintext weights (device functions):
//     out[v][r] = sum_{j<d} w[r][j] * ct[v][j]          v < nvec, r < nrows
// G1 sums of scalar multiples on level 1, products of powers in F_p^2 on level 2: the loop of MultConst + Add
// (bgn.go:253-291, :442-497) an encrypted weighted sum, a linear layer or EvalPoly / MultConstPoly is made of.
//
// The ciphertext vector is shared by all rows of w, so the work a scalar multiplication repeats per element is done
// once per ciphertext (Straus / Pippenger-style windows with a shared table):
//   1. k_lin_digits  recodes w into signed digits of omega bits (linrecode.hpp) and stores them as planes
//                    [window][column j][row r]: the lanes of a walk wave (consecutive r, one j) read consecutive bytes,
//                    never row-major w at stride d.
//   2. k_lin_table   one lane per ciphertext (v, j): the multiples 1 .. H = 2^(omega-1) — level 1 a chain of mixed
//                    additions made affine by ONE inversion per lane (Montgomery's trick), each entry with an identity
//                    flag; level 2 the powers c^1 .. c^H, one product each.  Entry m of column q = v*d + j is element
//                    q*H + (m-1) of a limb-major SoA, so a wave's gather of one limb touches at most H adjacent dwords.
//                    omega = 1 needs no table: the entries are the decoded elements.
//   3. k_lin_walk    one lane per (v, column chunk c, r), r fastest.  From the top window down: omega doublings
//                    (squarings) of the accumulator, then for every column of the chunk ONE table addition (product):
//                    the digit byte, the entry |digit|, negated (conjugated) for a negative digit.  A wave skips a
//                    column where none of its lanes has a digit.  The accumulator lives in the AGPR slots, the entry
//                    and the products' scratch in four LDS slots, as in polyops.hpp; the exceptional additions
//                    (accumulator equal to +- the entry, identity operands, the identity mid-run) are those of
//                    jac_add_affine and stay exact.  The next column's digit is requested before the current addition's
//                    products; its entry is not (2*NL more live registers: the 36-limb kernel would spill).
// A lane writes a plain canonical element; the host encodes it and, with more than one chunk, folds the chunks of an
// output with the passes of sumops.hpp.  Every output is a canonical encoding of a group element, so no byte depends
// on omega, the chunking or the order of accumulation.
#pragma once
#include "kernels.hpp"
#include "linrecode.hpp"
#include "ops.hpp"

namespace bgn {

// ---- digit planes ------------------------------------------------------------------------------------------------
// Thread i = j*nrows + r recodes w[r*d + j]; window t of it goes to element (t*d + j)*nrows + r of the planes.
__device__ __forceinline__ void lin_digits_lane(const LinDigitsArgs& A, size_t i) {
  const size_t j = i / A.nrows, r = i - j * A.nrows;
  int16_t dg[kLinMaxWindows];
  const int nwin = lin_recode(A.w[r * A.d + j], A.w_bits, A.omega, dg);
  const bool wide = lin_digit_bytes(A.omega) == 2;                          // uniform
#pragma unroll 1
  for (int t = 0; t < nwin; ++t) {
    const size_t at = ((size_t)t * A.d + j) * A.nrows + r;
    if (wide) reinterpret_cast<int16_t*>(A.planes)[at] = dg[t];
    else reinterpret_cast<int8_t*>(A.planes)[at] = (int8_t)dg[t];
  }
}

__device__ __forceinline__ int lin_digit_load(const uint8_t* planes, size_t at, bool wide) {
  return wide ? (int)reinterpret_cast<const int16_t*>(planes)[at] : (int)reinterpret_cast<const int8_t*>(planes)[at];
}

// ---- window tables -----------------------------------------------------------------------------------------------
// Level 1: entries 1*B .. H*B of column q, canonical Montgomery affine, each with an identity flag (an identity
// ciphertext, a point of small order).  tz, tp: one F_p per entry of scratch (the Z of the chain, the prefix products).
template <int NL>
__device__ __forceinline__ void lin_table_g1_lane(const LinTableArgs& A, size_t q, LFp<NL>* L,
                                                  const PairingConsts* __restrict__ C, const FpParams<NL>* __restrict__ P) {
  const int H = A.H;
  const size_t e0 = q * (size_t)H;                   // entry m at e0 + m - 1
  const size_t ts = A.st;
  const bool binf = A.cinf[q] != 0;
  JacAcc<NL> S;
  bool acc_inf = false;
  {
    Fp<NL> t;
    fp_set(t, P->one);
    a_store(S.T, t);
    a_store(S.U, t);
    a_store(S.Z, t);
    g_load(t, A.cx, A.sc, q);
    a_store(S.X, t);
    l_store(L + 2, t);
    g_store(A.tx, ts, e0, t);                    // 1*B
    g_load(t, A.cy, A.sc, q);
    a_store(S.Y, t);
    l_store(L + 3, t);
    g_store(A.ty, ts, e0, t);
    A.tinf[e0] = binf ? 1 : 0;
  }
  // 2B .. HB in Jacobian coordinates
#pragma unroll 1
  for (int m = 2; m <= H; ++m) {
    jac_add_affine<NL>(S, acc_inf, true, L, P);
    const bool inf = acc_inf || binf;
    Fp<NL> t;
    a_load(t, S.X);
    g_store(A.tx, ts, e0 + m - 1, t);
    a_load(t, S.Y);
    g_store(A.ty, ts, e0 + m - 1, t);
    a_load(t, S.Z);
    {
      Fp<NL> one;
      fp_set(one, P->one);
      fp_select(t, inf, one, t);                     // keep the shared inversion well defined
    }
    fp_reduce8(t, t, P);                             // Z <4 -> canonical
    g_store(A.tz, ts, e0 + m - 1, t);
    A.tinf[e0 + m - 1] = inf ? 1 : 0;
  }
  // one inversion for the H-1 Z (Montgomery's trick), then affine coordinates
  LFp<NL>* S0 = L;
  LFp<NL>* L1 = L + 1;
  Fp<NL> acc, r, u, inv;
  fp_set(acc, P->one);
#pragma unroll 1
  for (int m = 2; m <= H; ++m) {
    g_store(A.tp, ts, e0 + m - 1, acc);
    g_load(u, A.tz, ts, e0 + m - 1);
    l_store(L1, acc);
    fp_mul(r, L1, u, P);                             // <2
    fp_cond_sub_p<NL>(acc, r, P);
  }
  fp_inv<NL>(inv, acc, L, C, P);                     // <1   (uses L0, L1)
#pragma unroll 1
  for (int m = H; m >= 2; --m) {
    Fp<NL> zi;
    g_load(u, A.tp, ts, e0 + m - 1);
    l_store(L1, inv);
    fp_mul(zi, L1, u, P);                            // 1/Z_m <2
    g_load(u, A.tz, ts, e0 + m - 1);
    fp_mul(u, L1, u, P);                             // inverse of the shorter product <2
    fp_cond_sub_p<NL>(inv, u, P);
    l_store(L1, zi);
    fp_sqr(u, L1, zi, P);                            // zi^2 <2
    g_load(r, A.tx, ts, e0 + m - 1);                     // X <18
    fp_mulv(r, r, u, P, S0);                         // x <2   (36)
    fp_cond_sub_p<NL>(r, r, P);
    g_store(A.tx, ts, e0 + m - 1, r);
    fp_mul(u, L1, u, P);                             // zi^3 <2
    g_load(r, A.ty, ts, e0 + m - 1);                     // Y <18
    fp_mulv(r, r, u, P, S0);                         // y <2   (36)
    fp_cond_sub_p<NL>(r, r, P);
    g_store(A.ty, ts, e0 + m - 1, r);
  }
}

// Level 2: c^1 .. c^H, canonical Montgomery.
template <int NL>
__device__ __forceinline__ void lin_table_gt_lane(const LinTableArgs& A, size_t q, LFp<NL>* L,
                                                  const FpParams<NL>* __restrict__ P) {
  const size_t e0 = q * (size_t)A.H;
  AFp<NL> A0, A1;
  {
    Fp<NL> b0, b1;
    g_load(b0, A.cx, A.sc, q);
    g_load(b1, A.cy, A.sc, q);
    g_store(A.tx, A.st, e0, b0);
    g_store(A.ty, A.st, e0, b1);
    gt_set_multiplier<NL>(L, b0, b1);
    a_store(A0, b0);
    a_store(A1, b1);
  }
#pragma unroll 1
  for (int m = 2; m <= A.H; ++m) {
    gt_acc_mul<NL>(A0, A1, true, L, P);              // <4, <6
    Fp<NL> r, o;
    a_load(r, A0);
    fp_reduce8(o, r, P);
    g_store(A.tx, A.st, e0 + m - 1, o);
    a_load(r, A1);
    fp_reduce8(o, r, P);
    g_store(A.ty, A.st, e0 + m - 1, o);
  }
}

// ---- the walk ----------------------------------------------------------------------------------------------------
// What lane `lane` of the walk is: output (v, r), chunk c of the columns, which are j0 .. j1 - 1.
struct LinLane {
  size_t v, r, c, j0, j1;
};
__device__ __forceinline__ LinLane lin_lane(const LinWalkArgs& A, size_t lane) {
  LinLane l;
  const size_t vc = lane / A.nrows;
  l.r = lane - vc * A.nrows;
  l.v = vc / A.nchunk;
  l.c = vc - l.v * A.nchunk;
  l.j0 = l.c * A.d / A.nchunk;                       // nchunk <= d <= 2^28: no overflow, no empty chunk
  l.j1 = (l.c + 1) * A.d / A.nchunk;
  return l;
}

// y <- p - y (level 2: im) where neg, canonical either way
template <int NL>
__device__ __forceinline__ void lin_negate(Fp<NL>& y, bool neg, const FpParams<NL>* __restrict__ P) {
  Fp<NL> n;
  fp_neg<1>(n, y, P);
  fp_reduce8(n, n, P);
  fp_select(y, neg, n, y);
}

template <int NL>
__device__ __forceinline__ void lin_walk_g1_lane(const LinWalkArgs& A, size_t lane, bool live, LFp<NL>* L,
                                                 const PairingConsts* __restrict__ C, const FpParams<NL>* __restrict__ P) {
  const LinLane ln = lin_lane(A, lane);
  const bool wide = lin_digit_bytes(A.omega) == 2;
  const size_t steps = (A.d + A.nchunk - 1) / A.nchunk;                     // the longest chunk
  JacAcc<NL> S;
  {
    Fp<NL> t;
    fp_set(t, P->one);
    a_store(S.X, t);
    a_store(S.Y, t);
    a_store(S.T, t);
    a_store(S.U, t);
    fp_zero(t);
    a_store(S.Z, t);
  }
  bool acc_inf = true;
#pragma unroll 1
  for (int t = A.nwin - 1; t >= 0; --t) {
    if (t != A.nwin - 1) {
#pragma unroll 1
      for (int k = 0; k < A.omega; ++k) jac_double_checked<NL>(S, acc_inf, L, P);
    }
    const size_t plane = (size_t)t * A.d;
    int next = ln.j0 < ln.j1 ? lin_digit_load(A.planes, (plane + ln.j0) * A.nrows + ln.r, wide) : 0;
#pragma unroll 1
    for (size_t i = 0; i < steps; ++i) {
      const size_t j = ln.j0 + i;
      const int dg = next;
      next = j + 1 < ln.j1 ? lin_digit_load(A.planes, (plane + j + 1) * A.nrows + ln.r, wide) : 0;
      bool take = live && j < ln.j1 && dg != 0;
      const size_t e = take ? (ln.v * A.d + j) * (size_t)A.H + (size_t)((dg < 0 ? -dg : dg) - 1) : 0;
      if (take && A.tinf[e]) take = false;                                  // |dg| * ct = O: nothing to add
      if (!__ballot(take)) continue;
      Fp<NL> x;
      g_load(x, A.tx, A.st, e);
      l_store(L + 2, x);
      g_load(x, A.ty, A.st, e);
      lin_negate<NL>(x, dg < 0, P);
      l_store(L + 3, x);
      jac_add_affine<NL>(S, acc_inf, take, L, P);
    }
  }
  const size_t o = (ln.v * A.nrows + ln.r) * A.nchunk + ln.c;
  jac_store_affine<NL>(S, acc_inf, A.ox, A.oy, A.oinf, A.so, o, live, L, C, P);
}

template <int NL>
__device__ __forceinline__ void lin_walk_gt_lane(const LinWalkArgs& A, size_t lane, bool live, LFp<NL>* L,
                                                 const FpParams<NL>* __restrict__ P) {
  const LinLane ln = lin_lane(A, lane);
  const bool wide = lin_digit_bytes(A.omega) == 2;
  const size_t steps = (A.d + A.nchunk - 1) / A.nchunk;
  AFp<NL> A0, A1;
  {
    Fp<NL> t;
    fp_set(t, P->one);
    a_store(A0, t);
    fp_zero(t);
    a_store(A1, t);
  }
  bool started = false;
#pragma unroll 1
  for (int t = A.nwin - 1; t >= 0; --t) {
    if (t != A.nwin - 1 && __ballot(started)) {
#pragma unroll 1
      for (int k = 0; k < A.omega; ++k) {
        Fp<NL> a0, a1, s0, s1;
        a_load(a0, A0);
        a_load(a1, A1);
        fp2_sqr_v(s0, s1, a0, a1, P, L);             // <2, <4
        a_store(A0, s0);
        a_store(A1, s1);
      }
    }
    const size_t plane = (size_t)t * A.d;
    int next = ln.j0 < ln.j1 ? lin_digit_load(A.planes, (plane + ln.j0) * A.nrows + ln.r, wide) : 0;
#pragma unroll 1
    for (size_t i = 0; i < steps; ++i) {
      const size_t j = ln.j0 + i;
      const int dg = next;
      next = j + 1 < ln.j1 ? lin_digit_load(A.planes, (plane + j + 1) * A.nrows + ln.r, wide) : 0;
      const bool take = live && j < ln.j1 && dg != 0;
      if (!__ballot(take)) continue;
      const size_t e = take ? (ln.v * A.d + j) * (size_t)A.H + (size_t)((dg < 0 ? -dg : dg) - 1) : 0;
      Fp<NL> b0, b1;
      g_load(b0, A.tx, A.st, e);
      g_load(b1, A.ty, A.st, e);
      lin_negate<NL>(b1, dg < 0, P);                 // a negative digit: the conjugate, Neg on level 2
      gt_set_multiplier<NL>(L, b0, b1);
      gt_acc_mul<NL>(A0, A1, take, L, P);
      started = started || take;
    }
  }
  const size_t o = (ln.v * A.nrows + ln.r) * A.nchunk + ln.c;
  Fp<NL> r, x;
  a_load(r, A0);
  fp_from_mont<NL>(x, r, P, L);
  if (live) g_store<NL>(A.ox, A.so, o, x);
  a_load(r, A1);
  fp_from_mont<NL>(x, r, P, L);
  if (live) g_store<NL>(A.oy, A.so, o, x);
}

}  // namespace bgn
