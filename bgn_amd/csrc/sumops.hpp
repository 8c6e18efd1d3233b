// sumops.hpp — segmented sums of ciphertext arrays (device functions): out[s] = ct[s*len] + ... + ct[s*len + len - 1],
// the loop of Add the reference folds an array with (bgn.go:442-497; gadgets_test.go:24-46).
//
// One pass reduces nseg x len wire elements to nseg x split wire elements: lane (s, t), t < split, accumulates the
// elements t, t + split, t + 2 split, ... of segment s and writes partial t of that segment.  The host (engine.cpp
// sum_dev, planned by dispatch.hpp plan_sum) repeats the pass on the partials until split == 1.  Partials are canonical
// wire bytes, like the result: the group law is associative and commutative, so neither depends on the walk.
//
// Lanes and workgroups (SumGeom): with split >= FP_BLOCK a workgroup is FP_BLOCK consecutive lanes of ONE segment; with
// a smaller split it is floor(FP_BLOCK / split) whole segments.  Either way the lanes of a workgroup read, at step j,
// `split`-element runs that are contiguous in the array (one run per segment of the workgroup), and write one
// contiguous slice of partials.  The runs go through LDS (sum_stage_in) and are decoded in registers.
//   level 2: the accumulator and the element are plain residues, multiplied by barrett.hpp (sum_gt_step) — four Fp
//            live, the stage doubles as the product's scratch, no LDS product slots.  Beyond 40 limbs (no unrolled
//            Barrett product there) the Montgomery accumulator of ops.hpp (sum_gt_mont_step).
//   level 1: a Jacobian accumulator (ops.hpp JacAcc) takes each element by a mixed addition with the exceptional cases
//            resolved exactly — the element equal to the accumulator (doubling), its negative (identity mid-run), an
//            identity element, an identity accumulator — and is made affine once per lane per pass (sum_g1_finish).
#pragma once
#include "ops.hpp"
#include "codec.hpp"
#include "barrett.hpp"

namespace bgn {

// ---- geometry of a pass (host and device: the CPU tests walk it without a GPU) ---------------------------------
struct SumGeom {
  u32 spw;          // segments per workgroup (1 when split >= FP_BLOCK)
  u32 bps;          // workgroups per segment (1 when split < FP_BLOCK)
};
__host__ __device__ inline SumGeom sum_geom(u32 split) {
  SumGeom g;
  g.spw = split >= (u32)FP_BLOCK ? 1u : (u32)FP_BLOCK / split;
  g.bps = split >= (u32)FP_BLOCK ? (split + (u32)FP_BLOCK - 1) / (u32)FP_BLOCK : 1u;
  return g;
}
__host__ __device__ inline size_t sum_blocks(size_t nseg, u32 split) {
  const SumGeom g = sum_geom(split);
  return g.bps > 1 || g.spw == 1 ? nseg * g.bps : (nseg + g.spw - 1) / g.spw;
}
__host__ __device__ inline u32 sum_steps(u32 len, u32 split) { return (len + split - 1) / split; }

// What lane `tid` of workgroup `block` is in a pass: its segment and partial index, the first segment and the number
// of segments (runs) of its workgroup, the partial index its workgroup's first lane has, and how many lanes wide a run is.
struct SumLane {
  size_t seg, seg0;
  u32 t, t0, run, nruns, width;
  bool ok;          // the lane owns partial (seg, t)
};
__host__ __device__ inline SumLane sum_lane(size_t block, u32 tid, size_t nseg, u32 split) {
  const SumGeom g = sum_geom(split);
  SumLane l;
  if (split >= (u32)FP_BLOCK) {
    l.seg0 = l.seg = block / g.bps;
    l.t0 = (u32)(block % g.bps) * (u32)FP_BLOCK;
    l.t = l.t0 + tid;
    l.run = 0;
    l.nruns = 1;
    l.width = split - l.t0 < (u32)FP_BLOCK ? split - l.t0 : (u32)FP_BLOCK;
    l.ok = l.t < split;
  } else {
    l.seg0 = block * g.spw;
    l.run = tid / split;
    l.t = tid % split;
    l.t0 = 0;
    l.seg = l.seg0 + l.run;
    l.nruns = nseg - l.seg0 < (size_t)g.spw ? (u32)(nseg - l.seg0) : g.spw;
    l.width = split;
    l.ok = l.run < l.nruns;
  }
  return l;
}
// Elements each run of the workgroup holds at step j (the same for all its runs; 0: past the segment's end).
__host__ __device__ inline u32 sum_run_len(const SumLane& l, u32 j, u32 len, u32 split) {
  const size_t q = (size_t)j * split + l.t0;
  if (q >= len) return 0;
  return len - q < (size_t)l.width ? (u32)(len - q) : l.width;
}

// ---- staging ---------------------------------------------------------------------------------------------------
// The stage holds up to FP_BLOCK elements as one slice (WireStage) or as `nruns` runs, each at its own misalignment in
// a slot of `rsw` words: the aligned dwords of HBM and LDS coincide run by run.
template <int NL>
struct SumStage {
  static constexpr int WORDS = (WireStage<NL>::WORDS + 3 * FP_BLOCK + 3) / 4 * 4;
};
__host__ __device__ inline u32 sum_run_words(u32 split, size_t EB) { return (u32)((split * EB + 6) / 4 + 1); }

// HBM -> LDS for step j: run r of the workgroup is the n elements from element first + r * pitch of `in` on.  Returns
// the byte offset, inside the stage, of the calling lane's run.  Ends with a barrier.
template <int NL>
__device__ __forceinline__ u32 sum_stage_in(u32* w, const uint8_t* in, size_t first, size_t pitch, u32 nruns, u32 my_run,
                                            u32 n, u32 rsw, size_t EB) {
  if (nruns == 1) {                                        // workgroup-uniform
    return wire_stage_in<NL>(reinterpret_cast<WireStage<NL>*>(w), in + first * EB, (size_t)n * EB);
  }
  const u32 nb = n * (u32)EB;
  const u32 total = nruns * rsw;
  for (u32 base = threadIdx.x; base < total; base += 4 * FP_BLOCK) {
    u32 v[4];                                              // four loads in flight, then the four stores
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const u32 idx = base + (u32)k * FP_BLOCK;
      u32 t = 0;
      if (idx < total) {
        const u32 r = idx / rsw, i = idx - r * rsw;
        const uint8_t* g = in + (first + (size_t)r * pitch) * EB;
        const u32 mis = (u32)((uintptr_t)g & 3u);
        if (i < (mis + nb + 3) / 4) t = ((const u32*)(g - mis))[i];
      }
      v[k] = t;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const u32 idx = base + (u32)k * FP_BLOCK;
      if (idx < total) w[idx] = v[k];
    }
  }
  __syncthreads();
  const uint8_t* g = in + (first + (size_t)my_run * pitch) * EB;
  return my_run * rsw * 4u + (u32)((uintptr_t)g & 3u);
}

// The lane's element (plain residues) out of the stage, B = its first byte there.
template <int NL>
__device__ __forceinline__ void sum_decode(Fp<NL>& x, Fp<NL>& y, const u32* w, u32 B, int L) {
  if (StreamCodec<NL>::serves(L)) {                        // wave-uniform
    wire_to_limbs_stream<NL>(x, w, B, L);
    wire_to_limbs_stream<NL>(y, w, B + (u32)L, L);
  } else {
    const uint8_t* src = (const uint8_t*)w + B;
    wire_to_limbs<NL>(x, src, L);
    wire_to_limbs<NL>(y, src + L, L);
  }
}

// Lane `tid`'s result into the stage of the workgroup's slice of partials, which goes to `g` (any byte address).
template <int NL>
__device__ __forceinline__ void sum_encode(u32* w, const uint8_t* g, u32 tid, int L, const Fp<NL>& x, const Fp<NL>& y) {
  if (((uintptr_t)g & 3u) == 0 && StreamCodec<NL>::serves(L)) {      // workgroup-uniform: the slice is staged dword-aligned
    limbs_to_wire_stream<NL>(w, tid, L, x, y);
  } else {
    uint8_t* dst = (uint8_t*)w + ((uintptr_t)g & 3u) + (size_t)tid * (size_t)(2 * L);
    limbs_to_wire<NL>(dst, L, x);
    limbs_to_wire<NL>(dst + L, L, y);
  }
}

// ---- level 2: plain residues, Barrett products -------------------------------------------------------------------
// Residues at or above p (the wire format allows them) are reduced first, as k_gt_mul_wire does; an idle lane
// multiplies by 1.
template <int NL>
__device__ __forceinline__ void sum_gt_take(Fp<NL>& b0, Fp<NL>& b1, bool live, const FpParams<NL>* __restrict__ P,
                                            const BarrettParams<NL>* __restrict__ Bp) {
  const u32 pt = P->p[NL - 1];
  if (__ballot(!(b0.v[NL - 1] < pt && b1.v[NL - 1] < pt))) {
    if (__ballot(!(fp_lt_p(b0, P) && fp_lt_p(b1, P)))) {
      barrett_canon<NL>(b0, b0, P, Bp);
      barrett_canon<NL>(b1, b1, P, Bp);
    }
  }
  Fp<NL> one, zero;
  fp_zero(zero);
  fp_zero(one);
  one.v[0] = 1;
  fp_select(b0, live, b0, one);
  fp_select(b1, live, b1, zero);
}

// acc <- acc * b on canonical plain residues; sc: the lane's NL words of scratch (fp2_mul_plain).
template <int NL>
__device__ __forceinline__ void sum_gt_step(Fp<NL>& acc0, Fp<NL>& acc1, const Fp<NL>& b0, const Fp<NL>& b1,
                                            const FpParams<NL>* __restrict__ P, const BarrettParams<NL>* __restrict__ Bp,
                                            u32* __restrict__ sc, u32 sstride) {
  Fp<NL> r0, r1;
  fp2_mul_plain<NL>(r0, r1, acc0, acc1, b0, b1, false, P, Bp, sc, sstride);
  acc0 = r0;
  acc1 = r1;
}

// ---- level 2 beyond 40 limbs: the Montgomery accumulator of ops.hpp (A0 <4, A1 <6; slots L[0..3]) ----------------
template <int NL>
__device__ __forceinline__ void sum_gt_mont_init(AFp<NL>& A0, AFp<NL>& A1, const FpParams<NL>* __restrict__ P) {
  Fp<NL> t;
  fp_set(t, P->one);
  a_store(A0, t);
  fp_zero(t);
  a_store(A1, t);
}
template <int NL>
__device__ __forceinline__ void sum_gt_mont_step(AFp<NL>& A0, AFp<NL>& A1, const Fp<NL>& b0, const Fp<NL>& b1, bool live,
                                                 LFp<NL>* L, const FpParams<NL>* __restrict__ P) {
  if (!__ballot(live)) return;
  Fp<NL> m0, m1;
  fp_to_mont<NL>(m0, b0, P, L);            // <1, whatever residue came in
  fp_to_mont<NL>(m1, b1, P, L);
  gt_set_multiplier<NL>(L, m0, m1);
  gt_acc_mul<NL>(A0, A1, live, L, P);
}
template <int NL>
__device__ __forceinline__ void sum_gt_mont_finish(Fp<NL>& re, Fp<NL>& im, const AFp<NL>& A0, const AFp<NL>& A1,
                                                   LFp<NL>* L, const FpParams<NL>* __restrict__ P) {
  Fp<NL> t;
  a_load(t, A0);
  fp_from_mont<NL>(re, t, P, L);
  a_load(t, A1);
  fp_from_mont<NL>(im, t, P, L);
}

// ---- level 1: Jacobian accumulator (slots L[0..3]: L[0], L[1] scratch, L[2], L[3] the element) -------------------
template <int NL>
__device__ __forceinline__ void sum_g1_init(JacAcc<NL>& S, bool& acc_inf, const FpParams<NL>* __restrict__ P) {
  Fp<NL> t;
  fp_set(t, P->one);
  a_store(S.X, t);
  a_store(S.Y, t);
  a_store(S.T, t);
  a_store(S.U, t);
  fp_zero(t);
  a_store(S.Z, t);
  acc_inf = true;
}

// acc <- acc + (x, y) for a live lane; (x, y) plain canonical, all zero = the identity.
template <int NL>
__device__ __forceinline__ void sum_g1_step(JacAcc<NL>& S, bool& acc_inf, const Fp<NL>& x, const Fp<NL>& y, bool live,
                                            LFp<NL>* L, const FpParams<NL>* __restrict__ P) {
  const bool take = live && !(fp_is_zero_limbs(x) && fp_is_zero_limbs(y));
  if (!__ballot(take)) return;             // a wave of identities (or past the end): nothing to add
  Fp<NL> m;
  fp_to_mont<NL>(m, x, P, L);
  l_store(L + 2, m);
  fp_to_mont<NL>(m, y, P, L);
  l_store(L + 3, m);
  jac_add_affine<NL>(S, acc_inf, take, L, P);
}

// The accumulator as a plain canonical affine point (all zero: the identity); one inversion.
template <int NL>
__device__ __forceinline__ void sum_g1_finish(Fp<NL>& x, Fp<NL>& y, JacAcc<NL>& S, bool acc_inf, LFp<NL>* L,
                                              const PairingConsts* __restrict__ C, const FpParams<NL>* __restrict__ P) {
  Fp<NL> r, u, zi;
  a_load(r, S.Z);
  {
    Fp<NL> one;
    fp_set(one, P->one);
    fp_select(r, acc_inf, one, r);          // keep the inversion well defined
  }
  fp_reduce8(r, r, P);                      // <1 (Z <4)
  fp_inv<NL>(zi, r, L, C, P);               // <2   (uses L0, L1)
  l_store(L + 1, zi);
  fp_sqr(u, L + 1, zi, P);                  // zi^2 <2
  a_load(r, S.X);
  fp_mulv(r, r, u, P, L);                   // x <2   (36)
  fp_mul(u, L + 1, u, P);                   // zi^3 <2
  fp_from_mont<NL>(x, r, P, L);
  a_load(r, S.Y);
  fp_mulv(r, r, u, P, L);                   // y <2
  fp_from_mont<NL>(y, r, P, L);
  Fp<NL> zero;
  fp_zero(zero);
  fp_select(x, acc_inf, zero, x);
  fp_select(y, acc_inf, zero, y);
}

}  // namespace bgn
