// sparseops.hpp — sparse linear maps of ciphertext vectors with plaintext weights (device functions):
//     out[v][r] = sum_{e in row r} w[e] * ct[v][col[e]]          v < nvec, r < nrows
// over a compressed-row structure (row_ptr: nrows + 1 words, col and w: nnz words each) shared by all nvec vectors: a
// window over a series, a banded operator, a weighted group-by, a neighbour-list aggregation.  The recoding, the window
// tables, the exact additions and the folding of partials are those of the dense map (linops.hpp); what is new is the
// layout of the digits and the walk.
//   1. k_sp_digits  one thread per entry e: the signed digits of w[e] (linrecode.hpp), window t at planes[t*nnz_pad + e]
//                   — entry-major, so that a lane's run over its row reads consecutive bytes of one plane.  An entry
//                   whose column is not below d gets zero digits.
//   2. tables       k_lin_table_g1/gt over the nvec*d decoded ciphertexts, unchanged.
//   3. k_sp_walk    a workgroup is FP_BLOCK consecutive rows of one (vector v, chunk c).  It reads its FP_BLOCK + 1 words
//                   of row_ptr once, coalesced, into LDS; a lane takes its row's bounds from there, clips them to the
//                   contract (below) and takes chunk c's equal share, ceil(len / nchunk) entries.  The lanes' counts are
//                   reduced to the wave's maximum, which is the trip count of the inner loop: wave-uniform, so the
//                   additions of a wave stay in lockstep and a wave costs its longest row.  From the top window down:
//                   omega doublings (squarings) of the accumulator in the AGPR slots, then for i below the wave's
//                   maximum the lanes with i below their own count gather entry col*H + |digit| - 1 of the limb-major
//                   table, negate y (conjugate) for a negative digit and add — jac_add_affine with its exact
//                   exceptional cases on level 1, the F_p^2 product on level 2.  The next entry's column and digit are
//                   requested before the current addition's products; the table entry is not (linops.hpp says why).
// The contract on the index arrays, which the engine never scans on the host: row r is the entries row_ptr[r] ..
// row_ptr[r] + len - 1, len = min(row_ptr[r+1] - row_ptr[r], row_max) when row_ptr[r+1] > row_ptr[r] and 0 otherwise;
// an entry index >= nnz or a column >= d contributes nothing.  The lane clips [e0, e1) to nnz BEFORE it reads col or a
// digit, and tests the column against d BEFORE it forms a table address; a lane that takes no part in a step (a shorter
// row, a zero digit, a dropped entry, a lane past nrows) executes no load at all.
// A lane writes one plain canonical element at (v*nrows + r)*nchunk + c; the host encodes, folds the chunks with the
// passes of sumops.hpp and blinds, as for the dense map.  Rows are cut evenly and a wave costs its longest row: one
// giant row among short ones wastes lanes (splitting by entries across row boundaries is not done).
#pragma once
#include "linops.hpp"

namespace bgn {

// ---- digit planes ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void sp_digits_lane(const SpDigitsArgs& A, size_t e) {
  const bool in_range = (size_t)A.col[e] < A.d;
  int16_t dg[kLinMaxWindows];
  const int nwin = lin_recode(in_range ? A.w[e] : 0, A.w_bits, A.omega, dg);
  const bool wide = lin_digit_bytes(A.omega) == 2;                          // uniform
#pragma unroll 1
  for (int t = 0; t < nwin; ++t) {
    const size_t at = (size_t)t * A.nnz_pad + e;
    if (wide) reinterpret_cast<int16_t*>(A.planes)[at] = dg[t];
    else reinterpret_cast<int8_t*>(A.planes)[at] = (int8_t)dg[t];
  }
}

// ---- the walk ----------------------------------------------------------------------------------------------------
// What a lane of the walk is: output (v, r), chunk c, the entries e0 .. e0 + n - 1 (all below nnz), and the longest run
// of its wave.
struct SpLane {
  size_t v, r, c;
  u32 e0, n, wmax;
};

__device__ __forceinline__ u32 sp_wave_max(u32 x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const u32 y = (u32)__shfl_xor((int)x, off);
    x = y > x ? y : x;
  }
  return x;
}

// rp: the workgroup's row_ptr words, rp[i] = row_ptr[first row + i] for i <= FP_BLOCK (0 past nrows).
__device__ __forceinline__ SpLane sp_lane(const SpWalkArgs& A, size_t vc, size_t r, bool live, const u32* rp) {
  SpLane l;
  l.v = vc / A.nchunk;
  l.c = vc - l.v * A.nchunk;
  l.r = live ? r : A.nrows - 1;                      // keep the output index in range; nothing is stored
  const u32 a = rp[threadIdx.x], b = rp[threadIdx.x + 1];
  u32 len = (live && b > a) ? b - a : 0;
  if (len > A.row_max) len = A.row_max;              // entries past row_max are dropped
  if ((size_t)a >= A.nnz) len = 0;                   // ... and those past nnz: a + len <= nnz <= 2^28 from here on
  else if ((size_t)len > A.nnz - a) len = (u32)(A.nnz - a);
  const u32 nch = (u32)A.nchunk;
  const u32 per = (len + nch - 1) / nch;             // chunk c: [c*per, (c+1)*per) clipped to len
  const u64 lo = (u64)l.c * per, hi = lo + per;
  const u32 s0 = lo < len ? (u32)lo : len, s1 = hi < len ? (u32)hi : len;
  l.e0 = a + s0;
  l.n = s1 - s0;
  l.wmax = sp_wave_max(l.n);
  return l;
}

// The table entry of (v, col, digit) when the lane takes part in this step: nothing is formed from an unchecked index.
__device__ __forceinline__ bool sp_entry(const SpWalkArgs& A, const SpLane& ln, u32 i, u32 col, int dg, size_t& e) {
  const bool take = i < ln.n && dg != 0 && (size_t)col < A.d;
  e = take ? (ln.v * A.d + col) * (size_t)A.H + (size_t)((dg < 0 ? -dg : dg) - 1) : 0;
  return take;
}

template <int NL>
__device__ __forceinline__ void sp_walk_g1_lane(const SpWalkArgs& A, const SpLane& ln, bool live, LFp<NL>* L,
                                                const PairingConsts* __restrict__ C, const FpParams<NL>* __restrict__ P) {
  const bool wide = lin_digit_bytes(A.omega) == 2;
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
    const size_t plane = (size_t)t * A.nnz_pad + ln.e0;
    u32 ncol = 0;
    int ndg = 0;
    if (ln.n) {
      ncol = A.col[ln.e0];
      ndg = lin_digit_load(A.planes, plane, wide);
    }
#pragma unroll 1
    for (u32 i = 0; i < ln.wmax; ++i) {
      const u32 col = ncol;
      const int dg = ndg;
      ndg = 0;
      if (i + 1 < ln.n) {
        ncol = A.col[ln.e0 + i + 1];
        ndg = lin_digit_load(A.planes, plane + i + 1, wide);
      }
      size_t e;
      bool take = sp_entry(A, ln, i, col, dg, e);
      if (take && A.tinf[e]) take = false;                                  // |dg| * ct = O: nothing to add
      if (!__ballot(take)) continue;
      Fp<NL> x;
      fp_zero(x);
      if (take) g_load(x, A.tx, A.st, e);
      l_store(L + 2, x);
      if (take) g_load(x, A.ty, A.st, e);
      lin_negate<NL>(x, dg < 0, P);
      l_store(L + 3, x);
      jac_add_affine<NL>(S, acc_inf, take, L, P);
    }
  }
  const size_t o = (ln.v * A.nrows + ln.r) * A.nchunk + ln.c;
  jac_store_affine<NL>(S, acc_inf, A.ox, A.oy, A.oinf, A.so, o, live, L, C, P);
}

template <int NL>
__device__ __forceinline__ void sp_walk_gt_lane(const SpWalkArgs& A, const SpLane& ln, bool live, LFp<NL>* L,
                                                const FpParams<NL>* __restrict__ P) {
  const bool wide = lin_digit_bytes(A.omega) == 2;
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
    const size_t plane = (size_t)t * A.nnz_pad + ln.e0;
    u32 ncol = 0;
    int ndg = 0;
    if (ln.n) {
      ncol = A.col[ln.e0];
      ndg = lin_digit_load(A.planes, plane, wide);
    }
#pragma unroll 1
    for (u32 i = 0; i < ln.wmax; ++i) {
      const u32 col = ncol;
      const int dg = ndg;
      ndg = 0;
      if (i + 1 < ln.n) {
        ncol = A.col[ln.e0 + i + 1];
        ndg = lin_digit_load(A.planes, plane + i + 1, wide);
      }
      size_t e;
      const bool take = sp_entry(A, ln, i, col, dg, e);
      if (!__ballot(take)) continue;
      Fp<NL> b0, b1;
      fp_set(b0, P->one);                            // a lane that sits the step out multiplies nothing: any element
      fp_zero(b1);
      if (take) {
        g_load(b0, A.tx, A.st, e);
        g_load(b1, A.ty, A.st, e);
      }
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
