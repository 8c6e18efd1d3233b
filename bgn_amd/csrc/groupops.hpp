// groupops.hpp — the dense linear map of linops.hpp for NARROW weights (w_bits <= 4), shared over groups of columns
// instead of over the digits of one column (the multi-row form of Yao's method, "Four Russians"):
//     out[v][r] = sum_{j<d} w[r][j] * ct[v][j]
// With weights of one bit the window tables of linops.hpp cost every output d additions whatever the weights are.  Here g
// consecutive ciphertexts share one table of ALL their signed combinations sum tau_i * ct[j0 + i], tau in {-1, 0, 1}^g —
// M = (3^g - 1) / 2 entries up to sign — and an output pays one addition per group and bit plane: ceil(d / g) * w_bits.
//   1. k_grp_codes   one thread per (group, row) reads its g weights once and writes the balanced-ternary code of every
//                    bit plane (grprecode.hpp) to [plane][group][row], row fastest: the lanes of a walk wave (consecutive
//                    rows, one group) read consecutive 2-byte codes.
//   2. k_grp_table   one lane per group (v, G), level after level of the recurrence entry(c) = ct[j0 + k] + sign(c')
//                    entry(|c'|): level k is 3^k independent additions of two stored elements.  Level 1 (G1): affine +
//                    affine through the addition run of the fused Add (ops.hpp g1_add_run), which shares ONE inversion
//                    over the level's denominators — g inversions per group, not M — and keeps the exceptional additions
//                    exact by g1_classify: equal operands (two equal ciphertexts in a group: a doubling), opposite ones
//                    (the identity as an entry, flagged, which later levels add as such), an identity ciphertext.  Level 2
//                    (GT): one product in F_p^2 per entry, the conjugate for a negative c'.  Entry m of group q is element
//                    q*M + (m-1) of a limb-major SoA, so a wave's gather of one limb touches at most M adjacent dwords.
//   3. k_grp_walk    one lane per (v, chunk of whole groups, r), r fastest.  From the top plane down: one doubling
//                    (squaring), then per group of the chunk the code, and entry |code| added, negated (conjugated) for a
//                    negative code; a wave skips a group where all its lanes have code zero.  The working set is that of
//                    lin_walk_*_lane: accumulator in the AGPR slots, the entry and the products' scratch in four LDS
//                    slots, the next group's code requested before the current addition's products.
// The group's table is NOT staged in LDS: the four slots of a 256-lane workgroup already take most of a CU's LDS, and all
// the rows of a launch gather from the same few tens of KB per group, which the L2 serves.
// The lanes write plain canonical elements; the host encodes them and folds the chunks with the passes of sumops.hpp.
#pragma once
#include "grprecode.hpp"
#include "kernels.hpp"
#include "linops.hpp"
#include "ops.hpp"

namespace bgn {

// ---- codes -------------------------------------------------------------------------------------------------------
// Thread i = G*nrows + r.
__device__ __forceinline__ void grp_codes_lane(const GrpCodesArgs& A, size_t i) {
  const size_t G = i / A.nrows, r = i - G * A.nrows;
  const size_t j0 = G * (size_t)A.g;
  const int n = A.d - j0 < (size_t)A.g ? (int)(A.d - j0) : A.g;
  int16_t code[kGrpMaxBits];
  grp_codes(A.w + r * A.d + j0, n, A.w_bits, code);
#pragma unroll 1
  for (int t = 0; t < A.w_bits; ++t) A.codes[((size_t)t * A.ngroups + G) * A.nrows + r] = code[t];
}

// ---- group tables ------------------------------------------------------------------------------------------------
// Column k of group q = v*ngroups + G in the decoded vectors; `miss`: beyond the vector's end (then the last column's
// index, whose coordinates nothing uses).
__device__ __forceinline__ size_t grp_column(const GrpTableArgs& A, size_t q, int k, bool& miss) {
  const size_t v = q / A.ngroups, G = q - v * A.ngroups;
  const size_t col = G * (size_t)A.g + (size_t)k;
  miss = col >= A.d;
  return v * A.d + (miss ? A.d - 1 : col);
}

// Level k of the level-1 table as an addition run (ops.hpp g1_add_run): virtual element e = j*T + t is the j-th entry of
// the level in the group of lane t of the T lanes launched; a lane beyond the last group computes along on the last
// group's operands and stores nothing but its prefix products.  A = the group's column k, B = sign(c') entry(|c'|), the
// identity for c' = 0 and for a column beyond the vector's end.
template <int NL>
struct G1IoGrpLevel {
  const GrpTableArgs& A;
  int k;
  size_t T, nq;
  static constexpr bool kAbscissaLoads = false;
  __device__ __forceinline__ void where(size_t e, size_t& q, int& j) const {
    j = (int)(e / T);
    q = e - (size_t)j * T;
    if (q >= nq) q = nq - 1;
  }
  __device__ __forceinline__ void loadA(size_t e, Fp<NL>& x, Fp<NL>& y, bool& inf, const FpParams<NL>* __restrict__) const {
    size_t q;
    int j;
    where(e, q, j);
    bool miss;
    const size_t c = grp_column(A, q, k, miss);
    g_load(x, A.cx, A.sc, c);
    g_load(y, A.cy, A.sc, c);
    inf = miss || A.cinf[c] != 0;
  }
  __device__ __forceinline__ void loadB(size_t e, Fp<NL>& x, Fp<NL>& y, bool& inf, const FpParams<NL>* __restrict__ P) const {
    size_t q;
    int j;
    where(e, q, j);
    const int cp = grp_level_rest(k, j);
    const size_t at = q * (size_t)A.M + (size_t)((cp < 0 ? -cp : cp) - (cp != 0));      // c' = 0: entry 1, not used
    g_load(x, A.tx, A.st, at);
    g_load(y, A.ty, A.st, at);
    Fp<NL> ny;
    fp_neg<1>(ny, y, P);
    fp_reduce_lt<NL, 2>(ny, ny, P);           // p - 0 = p -> 0
    fp_select(y, cp < 0, ny, y);
    inf = cp == 0 || A.tinf[at] != 0;
  }
  __device__ __forceinline__ void store(size_t e, const Fp<NL>& x3, const Fp<NL>& y3, bool inf, LFp<NL>*,
                                        const FpParams<NL>* __restrict__ P) const {
    size_t q;
    int j;
    where(e, q, j);
    if (e - (size_t)j * T >= nq) return;
    const size_t at = q * (size_t)A.M + (size_t)(grp_level_entry(k, j) - 1);
    Fp<NL> o;
    fp_reduce_lt<NL, 4>(o, x3, P);            // x3 <4
    g_store(A.tx, A.st, at, o);
    fp_reduce_lt<NL, 4>(o, y3, P);            // y3 <3
    g_store(A.ty, A.st, at, o);
    A.tinf[at] = inf ? 1 : 0;
  }
};

// Level 1: lane t of T builds the table of group q = t (a lane beyond the last group: q is that group, live is false).
template <int NL>
__device__ __forceinline__ void grp_table_g1_lane(const GrpTableArgs& A, size_t q, bool live, size_t T, LFp<NL>* L,
                                                  const PairingConsts* __restrict__ C, const FpParams<NL>* __restrict__ P) {
  if (live) {                                         // level 0: entry 1 is column 0 (never beyond the end)
    bool miss;
    const size_t c = grp_column(A, q, 0, miss);
    Fp<NL> t;
    g_load(t, A.cx, A.sc, c);
    g_store(A.tx, A.st, q * (size_t)A.M, t);
    g_load(t, A.cy, A.sc, c);
    g_store(A.ty, A.st, q * (size_t)A.M, t);
    A.tinf[q * (size_t)A.M] = A.cinf[c];
  }
  G1IoGrpLevel<NL> io{A, 1, T, A.nvec * A.ngroups};
  int run = 3;
#pragma unroll 1
  for (int k = 1; k < A.g; ++k, run *= 3) {
    io.k = k;
    g1_add_run<NL, G1IoGrpLevel<NL>, false>(io, (size_t)run * T, run, A.tp, A.sp, L, C, P);
  }
}

// Level 2: the entries in ascending order, one product each; the multiplier of a level is its column.
template <int NL>
__device__ __forceinline__ void grp_table_gt_lane(const GrpTableArgs& A, size_t q, bool live, LFp<NL>* L,
                                                  const FpParams<NL>* __restrict__ P) {
  const size_t e0 = q * (size_t)A.M;
  int run = 1;
#pragma unroll 1
  for (int k = 0; k < A.g; ++k, run *= 3) {
    bool miss;
    const size_t c = grp_column(A, q, k, miss);
    Fp<NL> b0, b1;
    g_load(b0, A.cx, A.sc, c);
    g_load(b1, A.cy, A.sc, c);
    {
      Fp<NL> one, zero;
      fp_set(one, P->one);
      fp_zero(zero);
      fp_select(b0, miss, one, b0);                   // a column beyond the end: 1
      fp_select(b1, miss, zero, b1);
    }
    gt_set_multiplier<NL>(L, b0, b1);
#pragma unroll 1
    for (int j = 0; j < run; ++j) {
      const int cp = grp_level_rest(k, j);
      const size_t at = e0 + (size_t)(run + cp - 1);
      if (cp == 0) {
        if (live) {
          g_store(A.tx, A.st, at, b0);
          g_store(A.ty, A.st, at, b1);
        }
        continue;
      }
      Fp<NL> r, o;
      AFp<NL> A0, A1;
      g_load(r, A.tx, A.st, e0 + (size_t)((cp < 0 ? -cp : cp) - 1));
      a_store(A0, r);
      g_load(r, A.ty, A.st, e0 + (size_t)((cp < 0 ? -cp : cp) - 1));
      lin_negate<NL>(r, cp < 0, P);                   // the conjugate: the inverse on GT
      a_store(A1, r);
      gt_acc_mul<NL>(A0, A1, true, L, P);             // <4, <6
      a_load(r, A0);
      fp_reduce8(o, r, P);
      if (live) g_store(A.tx, A.st, at, o);
      a_load(r, A1);
      fp_reduce8(o, r, P);
      if (live) g_store(A.ty, A.st, at, o);
    }
  }
}

// ---- the walk ----------------------------------------------------------------------------------------------------
// What lane `lane` of the walk is: output (v, r), chunk c of the groups, which are G0 .. G1 - 1.
struct GrpLane {
  size_t v, r, c, G0, G1;
};
__device__ __forceinline__ GrpLane grp_lane(const GrpWalkArgs& A, size_t lane) {
  GrpLane l;
  const size_t vc = lane / A.nrows;
  l.r = lane - vc * A.nrows;
  l.v = vc / A.nchunk;
  l.c = vc - l.v * A.nchunk;
  l.G0 = l.c * A.ngroups / A.nchunk;                 // nchunk <= ngroups <= 2^28: no overflow, no empty chunk
  l.G1 = (l.c + 1) * A.ngroups / A.nchunk;
  return l;
}

template <int NL>
__device__ __forceinline__ void grp_walk_g1_lane(const GrpWalkArgs& A, size_t lane, bool live, LFp<NL>* L,
                                                 const PairingConsts* __restrict__ C, const FpParams<NL>* __restrict__ P) {
  const GrpLane ln = grp_lane(A, lane);
  const size_t steps = (A.ngroups + A.nchunk - 1) / A.nchunk;               // the longest chunk
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
  for (int t = A.w_bits - 1; t >= 0; --t) {
    if (t != A.w_bits - 1) jac_double_checked<NL>(S, acc_inf, L, P);
    const size_t plane = (size_t)t * A.ngroups;
    int next = A.codes[(plane + ln.G0) * A.nrows + ln.r];
#pragma unroll 1
    for (size_t i = 0; i < steps; ++i) {
      const size_t G = ln.G0 + i;
      const int cd = next;
      next = G + 1 < ln.G1 ? (int)A.codes[(plane + G + 1) * A.nrows + ln.r] : 0;
      bool take = live && G < ln.G1 && cd != 0;
      const size_t e = take ? (ln.v * A.ngroups + G) * (size_t)A.M + (size_t)((cd < 0 ? -cd : cd) - 1) : 0;
      if (take && A.tinf[e]) take = false;                                  // the combination is O: nothing to add
      if (!__ballot(take)) continue;
      Fp<NL> x;
      g_load(x, A.tx, A.st, e);
      l_store(L + 2, x);
      g_load(x, A.ty, A.st, e);
      lin_negate<NL>(x, cd < 0, P);
      l_store(L + 3, x);
      jac_add_affine<NL>(S, acc_inf, take, L, P);
    }
  }
  const size_t o = (ln.v * A.nrows + ln.r) * A.nchunk + ln.c;
  jac_store_affine<NL>(S, acc_inf, A.ox, A.oy, A.oinf, A.so, o, live, L, C, P);
}

template <int NL>
__device__ __forceinline__ void grp_walk_gt_lane(const GrpWalkArgs& A, size_t lane, bool live, LFp<NL>* L,
                                                 const FpParams<NL>* __restrict__ P) {
  const GrpLane ln = grp_lane(A, lane);
  const size_t steps = (A.ngroups + A.nchunk - 1) / A.nchunk;
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
  for (int t = A.w_bits - 1; t >= 0; --t) {
    if (t != A.w_bits - 1 && __ballot(started)) {
      Fp<NL> a0, a1, s0, s1;
      a_load(a0, A0);
      a_load(a1, A1);
      fp2_sqr_v(s0, s1, a0, a1, P, L);               // <2, <4
      a_store(A0, s0);
      a_store(A1, s1);
    }
    const size_t plane = (size_t)t * A.ngroups;
    int next = A.codes[(plane + ln.G0) * A.nrows + ln.r];
#pragma unroll 1
    for (size_t i = 0; i < steps; ++i) {
      const size_t G = ln.G0 + i;
      const int cd = next;
      next = G + 1 < ln.G1 ? (int)A.codes[(plane + G + 1) * A.nrows + ln.r] : 0;
      const bool take = live && G < ln.G1 && cd != 0;
      if (!__ballot(take)) continue;
      const size_t e = take ? (ln.v * A.ngroups + G) * (size_t)A.M + (size_t)((cd < 0 ? -cd : cd) - 1) : 0;
      Fp<NL> b0, b1;
      g_load(b0, A.tx, A.st, e);
      g_load(b1, A.ty, A.st, e);
      lin_negate<NL>(b1, cd < 0, P);                 // a negative code: the conjugate, Neg on level 2
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
