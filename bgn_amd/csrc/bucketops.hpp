// bucketops.hpp — the bucket method (Pippenger) for the dense linear map of linops.hpp (device functions):
//     out[v][r] = sum_{j<d} w[r][j] * ct[v][j]
// without a table of multiples: the half of "Straus / Pippenger-style windows" that pays for ONE or a few rows over a very
// long vector, where no row shares a ciphertext's table and every column would pay (H - 1) table steps for nothing.
//
// For window t of row r, column j belongs to bucket |digit_t(w[r][j])| with the digit's sign; the window's value is
// sum_b b * B_b over the bucket sums B_b, and the windows are combined by doublings.  A column costs nwin additions at a
// WIDE window (3 at 16-bit weights and 8-bit digits) and no table step.  A lane cannot own private buckets (one is 288
// bytes at a 1024-bit key, and a lane's run is about 16 columns), so the columns are sorted by digit and the buckets
// are shared by all lanes:
//   1. k_bkt_count    one thread per (r, j): recode w[r][j] (linrecode.hpp) and count the nonzero digit of every window
//                     into the histogram cnt[r][t][b], b = |digit| - 1 — in LDS first (a workgroup holds columns of one
//                     row: nwin * H <= 512 bins), then one vector atomic add per bin the workgroup touched.
//   2. k_bkt_offsets  one workgroup scans the nb = nrows * nwin * H counts.  A bucket's list is rounded up to whole runs
//                     of R entries, so every run lies in exactly one bucket; the scan leaves the first run of every bucket
//                     (a lane finds the bucket of its run by bisection over these, a few cached loads) and the bucket's
//                     count for the NEXT pass, which is its number of runs — for all the passes at once.  Nothing is read
//                     back: the host launches the bound nrows * nwin * (ceil(d / R) + H) of runs, and a wave whose runs
//                     are all past the live ones exits before any load.
//   3. k_bkt_scatter  again one thread per (r, j), the digits recomputed (a few integer instructions): per window a slot
//                     of the bucket's list from an atomic cursor, j | sign << 31 stored there (d <= 2^28).  The padding
//                     of a list is never read: a run knows how many of its R slots are live from the bucket's count.
//                     The order inside a bucket depends on the atomics and no byte of the result on that order.
//   4. k_bkt_reduce   one lane per (vector v, run): the run's columns gathered by index from the decoded limb-major SoA,
//                     y negated (level 2: the conjugate) for a set sign bit, accumulated as the walk of linops.hpp does —
//                     the accumulator in the AGPR slots, operand and scratch in the four LDS slots, the next entry's
//                     index requested before the current addition's products; level 1 by jac_add_affine with its exact
//                     exceptional cases (an identity operand, P + P, P + (-P) mid-run) and ONE inversion per lane that
//                     makes the partial affine again (an identity partial carries its flag), level 2 by the F_p^2 product.
//                     Later passes reduce the partials of a bucket, which are contiguous, the same way; ceil(log_R d)
//                     passes leave at most one element per bucket.
//   5. k_bkt_fold     sum_b b * B_b = sum_k 2^k * (sum of the B_b with bit k of b set): only mixed additions of affine
//                     elements, so the exceptional cases stay those of jac_add_affine.  Stage 1: one lane per (v, r, t, bit
//                     k, group of g buckets); stage 2 (more than one group): one lane per (v, r, t, k) adds the groups;
//                     stage 3: one lane per output walks the nwin * omega bit sums from the top, a doubling and an addition
//                     each, and writes the plain canonical result.  Dependent depth g + H/g additions and two conversions,
//                     then nwin * omega (doubling + addition): below the 2g + 2H/g general additions, log2 g doublings and
//                     nwin * (omega doublings + addition) of a running-sum fold in two levels.
// Every output is a canonical encoding of a group element: no byte depends on the window, on R or on the path.
#pragma once
#include "kernels.hpp"
#include "linops.hpp"

namespace bgn {

constexpr int kBktMaxBins = 512;          // nwin * H at most: omega = 8, w_bits = 31
constexpr int kBktScanBlock = 1024;

// ---- the sort ----------------------------------------------------------------------------------------------------
// Workgroup (r, block of FP_BLOCK columns).  `h`: kBktMaxBins words of LDS.
__device__ __forceinline__ void bkt_count_block(const BktSortArgs& A, u32* h) {
  const int H = 1 << (A.omega - 1), bins = A.nwin * H;
  const size_t nblk = (A.d + FP_BLOCK - 1) / FP_BLOCK;
  const size_t r = (size_t)blockIdx.x / nblk, j = ((size_t)blockIdx.x - r * nblk) * FP_BLOCK + threadIdx.x;
  for (int i = threadIdx.x; i < bins; i += FP_BLOCK) h[i] = 0;
  __syncthreads();
  if (j < A.d) {
    int16_t dg[kLinMaxWindows];
    const int nwin = lin_recode(A.w[r * A.d + j], A.w_bits, A.omega, dg);
#pragma unroll 1
    for (int t = 0; t < nwin; ++t)
      if (dg[t]) atomicAdd(&h[t * H + (dg[t] < 0 ? -dg[t] : dg[t]) - 1], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < bins; i += FP_BLOCK)
    if (h[i]) atomicAdd(&A.cnt[r * (size_t)bins + i], h[i]);
}

__device__ __forceinline__ void bkt_scatter_lane(const BktSortArgs& A) {
  const int H = 1 << (A.omega - 1), bins = A.nwin * H;
  const size_t nblk = (A.d + FP_BLOCK - 1) / FP_BLOCK;
  const size_t r = (size_t)blockIdx.x / nblk, j = ((size_t)blockIdx.x - r * nblk) * FP_BLOCK + threadIdx.x;
  if (j >= A.d) return;
  int16_t dg[kLinMaxWindows];
  const int nwin = lin_recode(A.w[r * A.d + j], A.w_bits, A.omega, dg);
#pragma unroll 1
  for (int t = 0; t < nwin; ++t) {
    if (!dg[t]) continue;
    const u32 slot = atomicAdd(&A.cnt[r * (size_t)bins + t * H + (dg[t] < 0 ? -dg[t] : dg[t]) - 1], 1u);
    A.ent[slot] = (u32)j | (dg[t] < 0 ? 0x80000000u : 0u);
  }
}

// One workgroup of kBktScanBlock threads; thread i owns the buckets [i*per, (i+1)*per).  `part`: kBktScanBlock words.
__device__ __forceinline__ void bkt_offsets_block(const BktOffsetsArgs& A, u32* part) {
  const u32 tid = threadIdx.x;
  const size_t per = (A.nb + kBktScanBlock - 1) / kBktScanBlock;
  const size_t b0 = tid * per < A.nb ? tid * per : A.nb, b1 = b0 + per < A.nb ? b0 + per : A.nb;
#pragma unroll 1
  for (int p = 0; p < A.npass; ++p) {
    const u32* c = A.cnt + (size_t)p * A.nb;
    u32* cn = A.cnt + (size_t)(p + 1) * A.nb;
    u32* rs = A.rs + (size_t)p * A.nb;
    u32 sum = 0;
    for (size_t b = b0; b < b1; ++b) sum += (c[b] + A.R - 1) / A.R;
    part[tid] = sum;
    __syncthreads();
    for (u32 off = 1; off < (u32)kBktScanBlock; off <<= 1) {                  // inclusive scan of the threads' sums
      const u32 below = tid >= off ? part[tid - off] : 0;
      __syncthreads();
      part[tid] += below;
      __syncthreads();
    }
    u32 run = part[tid] - sum;
    for (size_t b = b0; b < b1; ++b) {
      const u32 n = (c[b] + A.R - 1) / A.R;
      rs[b] = run;
      cn[b] = n;
      if (p == 0) A.cur[b] = run * A.R;
      run += n;
    }
    __syncthreads();
  }
}

// ---- what a lane sums ----------------------------------------------------------------------------------------------
// A source names the elements of one lane: at(i, e, neg) for i < steps — whether step i has an element, its index in
// the source SoA (below its stride: nothing is formed from an unchecked index) and whether it enters negated.

// The run of a reduce lane.
struct BktRunSrc {
  const u32* ent;      // pass 0: the run's R slots; null: the partials from e0 on
  size_t e0, sper;
  u32 n;               // live elements of the run (0: a run past the live ones, or a lane past the launch)
  __device__ __forceinline__ bool at(u32 i, u32& e, bool& neg) const {
    neg = false;
    if (i >= n) return false;
    if (!ent) {
      e = (u32)(e0 + i);
      return true;
    }
    const u32 w = ent[i];
    const u32 j = w & 0x7fffffffu;
    neg = (w >> 31) != 0;
    e = (u32)(e0 + j);
    return j < sper;
  }
};

__device__ __forceinline__ BktRunSrc bkt_run(const BktReduceArgs& A, size_t lane, bool live) {
  const size_t v = lane / A.nruns, run = lane - v * A.nruns;
  size_t lo = 0, hi = A.nb;                            // the first bucket that starts after `run` ...
  while (lo < hi) {
    const size_t mid = (lo + hi) / 2;
    if ((size_t)A.rs[mid] <= run) lo = mid + 1;
    else hi = mid;
  }
  const size_t b = lo ? lo - 1 : 0;                    // ... follows the run's: an empty bucket starts where the next does
  const u64 first = (u64)(run - A.rs[b]) * A.R;        // (rs[0] = 0 <= run)
  const u32 c = A.cnt[b];
  BktRunSrc s;
  s.n = live && first < c ? (c - first < A.R ? (u32)(c - first) : A.R) : 0;
  s.ent = A.ent ? A.ent + run * A.R : nullptr;
  s.e0 = A.ent ? v * A.sper : v * A.sper + A.prs[b] + (size_t)first;
  s.sper = A.sper;
  return s;
}

// The buckets (stage 1) or group sums (stage 2) of a fold lane.
struct BktFoldSrc {
  const u32* cnt; const u32* rs;    // stage 1, at the lane's window; null on stage 2
  size_t e0;
  u32 b0, n, bit;
  __device__ __forceinline__ bool at(u32 i, u32& e, bool& neg) const {
    neg = false;
    if (i >= n) return false;
    if (!cnt) {
      e = (u32)(e0 + i);
      return true;
    }
    const u32 b = b0 + i;                              // bucket b holds the digit b + 1
    if (!(((b + 1) >> bit) & 1u) || !cnt[b]) return false;
    e = (u32)(e0 + rs[b]);
    return true;
  }
};

__device__ __forceinline__ BktFoldSrc bkt_fold_src(const BktFoldArgs& A, size_t lane, bool live) {
  BktFoldSrc s;
  if (A.stage == 2) {
    s.cnt = s.rs = nullptr;
    s.e0 = lane * (size_t)A.nc;
    s.b0 = s.bit = 0;
    s.n = live ? (u32)A.nc : 0;
    return s;
  }
  const int H = 1 << (A.omega - 1);
  const size_t q = lane / (size_t)A.nc, c = lane - q * A.nc;          // q = ((v*nrows + r)*nwin + t)*omega + k
  const size_t vrt = q / (size_t)A.omega, rt = vrt % (A.nrows * (size_t)A.nwin), v = vrt / (A.nrows * (size_t)A.nwin);
  s.bit = (u32)(q - vrt * A.omega);
  s.b0 = (u32)(c * A.g);
  s.n = live ? ((u32)H - s.b0 < (u32)A.g ? (u32)H - s.b0 : (u32)A.g) : 0;
  s.cnt = A.cnt + rt * H;
  s.rs = A.rs + rt * H;
  s.e0 = v * A.sper;
  return s;
}

// ---- level 1 -------------------------------------------------------------------------------------------------------
template <int NL>
__device__ __forceinline__ void bkt_acc_init_g1(JacAcc<NL>& S, const FpParams<NL>* __restrict__ P) {
  Fp<NL> t;
  fp_set(t, P->one);
  a_store(S.X, t);
  a_store(S.Y, t);
  a_store(S.T, t);
  a_store(S.U, t);
  fp_zero(t);
  a_store(S.Z, t);
}

// acc <- acc +- element e of the source where take (an identity element adds nothing)
template <int NL>
__device__ __forceinline__ void bkt_add_g1(const BktIo& io, JacAcc<NL>& S, bool& acc_inf, bool take, u32 e, bool neg,
                                           LFp<NL>* L, const FpParams<NL>* __restrict__ P) {
  if (take && io.sinf[e]) take = false;
  if (!__ballot(take)) return;
  Fp<NL> x;
  fp_zero(x);
  if (take) g_load(x, io.sx, io.ss, e);
  l_store(L + 2, x);
  if (take) g_load(x, io.sy, io.ss, e);
  lin_negate<NL>(x, neg, P);
  l_store(L + 3, x);
  jac_add_affine<NL>(S, acc_inf, take, L, P);
}

// Jacobian accumulator -> canonical Montgomery affine with its identity flag: one inversion per lane.
template <int NL>
__device__ __forceinline__ void bkt_store_g1(JacAcc<NL>& S, bool is_inf, const BktIo& io, size_t o, bool store, LFp<NL>* L,
                                             const PairingConsts* __restrict__ C, const FpParams<NL>* __restrict__ P) {
  Fp<NL> r, u, zi;
  a_load(r, S.Z);
  {
    Fp<NL> one;
    fp_set(one, P->one);
    fp_select(r, is_inf, one, r);           // keep the inversion well defined
  }
  fp_reduce8(r, r, P);                      // <1 (Z <4)
  fp_inv<NL>(zi, r, L, C, P);               // <2   (uses L0, L1)
  l_store(L + 1, zi);
  fp_sqr(u, L + 1, zi, P);                  // zi^2 <2
  a_load(r, S.X);
  fp_mulv(r, r, u, P, L);                   // x <2   (36)
  fp_cond_sub_p<NL>(r, r, P);
  if (store) g_store(io.ox, io.so, o, r);
  fp_mul(u, L + 1, u, P);                   // zi^3 <2
  a_load(r, S.Y);
  fp_mulv(r, r, u, P, L);                   // y <2
  fp_cond_sub_p<NL>(r, r, P);
  if (store) g_store(io.oy, io.so, o, r);
  if (store) io.oinf[o] = is_inf ? 1 : 0;
}

// The sum of a source's elements into partial o.
template <int NL, class Src>
__device__ __forceinline__ void bkt_sum_g1(const Src& src, u32 steps, const BktIo& io, size_t o, bool store, LFp<NL>* L,
                                           const PairingConsts* __restrict__ C, const FpParams<NL>* __restrict__ P) {
  JacAcc<NL> S;
  bkt_acc_init_g1<NL>(S, P);
  bool acc_inf = true;
  u32 ne = 0;
  bool nneg = false, ntake = src.at(0, ne, nneg);
#pragma unroll 1
  for (u32 i = 0; i < steps; ++i) {
    const u32 e = ne;
    const bool neg = nneg, take = ntake;
    ntake = src.at(i + 1, ne, nneg);                  // requested before this addition's products
    bkt_add_g1<NL>(io, S, acc_inf, take, take ? e : 0, neg, L, P);
  }
  bkt_store_g1<NL>(S, acc_inf, io, o, store, L, C, P);
}

// Output o = sum_s 2^s * element o*nbits + s, plain canonical.
template <int NL>
__device__ __forceinline__ void bkt_horner_g1(const BktFoldArgs& A, size_t o, bool live, LFp<NL>* L,
                                              const PairingConsts* __restrict__ C, const FpParams<NL>* __restrict__ P) {
  const int nbits = A.nwin * A.omega;
  JacAcc<NL> S;
  bkt_acc_init_g1<NL>(S, P);
  bool acc_inf = true;
#pragma unroll 1
  for (int s = nbits - 1; s >= 0; --s) {
    if (s != nbits - 1) jac_double_checked<NL>(S, acc_inf, L, P);
    bkt_add_g1<NL>(A.io, S, acc_inf, live, (u32)(o * nbits + s), false, L, P);
  }
  jac_store_affine<NL>(S, acc_inf, A.io.ox, A.io.oy, A.io.oinf, A.io.so, o, live, L, C, P);
}

// ---- level 2 -------------------------------------------------------------------------------------------------------
template <int NL>
__device__ __forceinline__ void bkt_acc_init_gt(AFp<NL>& A0, AFp<NL>& A1, const FpParams<NL>* __restrict__ P) {
  Fp<NL> t;
  fp_set(t, P->one);
  a_store(A0, t);
  fp_zero(t);
  a_store(A1, t);
}

// acc <- acc * element e of the source (its conjugate where neg) where take
template <int NL>
__device__ __forceinline__ void bkt_mul_gt(const BktIo& io, AFp<NL>& A0, AFp<NL>& A1, bool take, u32 e, bool neg,
                                           LFp<NL>* L, const FpParams<NL>* __restrict__ P) {
  if (!__ballot(take)) return;
  Fp<NL> b0, b1;
  fp_zero(b0);
  fp_zero(b1);
  if (take) g_load(b0, io.sx, io.ss, e);
  if (take) g_load(b1, io.sy, io.ss, e);
  lin_negate<NL>(b1, neg, P);
  gt_set_multiplier<NL>(L, b0, b1);
  gt_acc_mul<NL>(A0, A1, take, L, P);
}

template <int NL, class Src>
__device__ __forceinline__ void bkt_sum_gt(const Src& src, u32 steps, const BktIo& io, size_t o, bool store, LFp<NL>* L,
                                           const FpParams<NL>* __restrict__ P) {
  AFp<NL> A0, A1;
  bkt_acc_init_gt<NL>(A0, A1, P);
  u32 ne = 0;
  bool nneg = false, ntake = src.at(0, ne, nneg);
#pragma unroll 1
  for (u32 i = 0; i < steps; ++i) {
    const u32 e = ne;
    const bool neg = nneg, take = ntake;
    ntake = src.at(i + 1, ne, nneg);
    bkt_mul_gt<NL>(io, A0, A1, take, take ? e : 0, neg, L, P);
  }
  Fp<NL> r, x;
  a_load(r, A0);                                     // <4
  fp_reduce8(x, r, P);
  if (store) g_store<NL>(io.ox, io.so, o, x);
  a_load(r, A1);                                     // <6
  fp_reduce8(x, r, P);
  if (store) g_store<NL>(io.oy, io.so, o, x);
}

template <int NL>
__device__ __forceinline__ void bkt_horner_gt(const BktFoldArgs& A, size_t o, bool live, LFp<NL>* L,
                                              const FpParams<NL>* __restrict__ P) {
  const int nbits = A.nwin * A.omega;
  AFp<NL> A0, A1;
  bkt_acc_init_gt<NL>(A0, A1, P);
#pragma unroll 1
  for (int s = nbits - 1; s >= 0; --s) {
    if (s != nbits - 1) {
      Fp<NL> a0, a1, s0, s1;
      a_load(a0, A0);
      a_load(a1, A1);
      fp2_sqr_v(s0, s1, a0, a1, P, L);               // <2, <4
      a_store(A0, s0);
      a_store(A1, s1);
    }
    bkt_mul_gt<NL>(A.io, A0, A1, live, (u32)(o * nbits + s), false, L, P);
  }
  Fp<NL> r, x;
  a_load(r, A0);
  fp_from_mont<NL>(x, r, P, L);
  if (live) g_store<NL>(A.io.ox, A.io.so, o, x);
  a_load(r, A1);
  fp_from_mont<NL>(x, r, P, L);
  if (live) g_store<NL>(A.io.oy, A.io.so, o, x);
}

}  // namespace bgn
