// scanops.hpp — prefix sums of ciphertext arrays (device functions): out[s*len + i] = ct[s*len] + ... + ct[s*len + i],
// the inclusive scan of every segment — G1 addition on level 1, the F_p^2 product on level 2.
//
// Reduce, then scan (engine.cpp scan_dev, planned by dispatch.hpp plan_scan).  A segment is cut into chunks of c
// consecutive elements (its last chunk may be shorter) and ONE LANE OWNS ONE CHUNK: lane q = s * nch + k walks the
// elements s*len + k*c + j, j = 0, 1, ...  A first launch in totals-only mode leaves every chunk's total as wire
// bytes; the host scans those per segment with the same two launches, one recursion level down, until a segment's
// totals are one chunk; the apply launch then starts every lane from its offset — the scanned total of the chunk in
// front of it, the identity for a segment's first chunk — and emits one prefix per element.  Every prefix is canonical
// wire bytes of a group element, so no byte depends on c.
//
// Data movement.  At step j the lanes of a workgroup need FP_BLOCK rows that lie a chunk apart (and closer at a
// segment's end): every lane puts the element index of its row into a table in LDS (SCAN_NONE: no row), and the
// workgroup moves the rows between HBM and per-row slots of the stage with whole-row coalesced dword accesses
// (scan_stage_in, scan_stage_out), every row at its own misalignment so that the aligned dwords of HBM and LDS
// coincide.  An element is 2L bytes; with L odd neighbouring rows share a dword, and the neighbour belongs to another
// step of the same lane or to the next lane, which may have written it already: scan_stage_out writes the dwords that
// lie wholly inside the row as dwords and the edge bytes as bytes, never a byte of another row.
//
// Level 2: one fp2_mul_plain per element on plain residues (sumops.hpp sum_gt_step), the product is the output.
// Level 1: the additions of a lane depend on each other, so the shared inversion of k_g1_add_wire has nothing to share
// along the run; two sweeps inside one launch share it instead.  Forward: jac_add_affine per element, every Jacobian
// prefix (X, Y, Z) and the running product of the Zs limb-major in the workspace (an identity prefix stores X = Y = 0
// and Z = 1: it comes out as all zeros without a flag).  One fp_inv per lane.  Backward: 1/Z_j peeled off the inverted
// product, x = X zi^2, y = Y zi^3, encoded and written.  One inversion per lane-run, not one per output.
#pragma once
#include "kernels.hpp"
#include "sumops.hpp"

namespace bgn {

constexpr u32 SCAN_NONE = 0xFFFFFFFFu;

// ---- the lane's chunk (ScanArgs: kernels.hpp) --------------------------------------------------------------------
struct ScanLane {
  u32 e0;           // element index of the chunk's first element
  u32 n;            // its length (0: no chunk)
  u32 prev;         // row of `off` the chunk starts from (SCAN_NONE: the identity)
};
__host__ __device__ inline ScanLane scan_lane(size_t q, size_t q1, u32 len, u32 c, u32 nch) {
  ScanLane l;
  l.e0 = 0;
  l.n = 0;
  l.prev = SCAN_NONE;
  if (q >= q1) return l;
  const size_t seg = q / nch;
  const u32 k = (u32)(q - seg * nch);
  l.e0 = (u32)(seg * len + (size_t)k * c);
  l.n = len - k * c < c ? len - k * c : c;
  if (k) l.prev = (u32)(q - 1);
  return l;
}

// ---- staging: FP_BLOCK rows, row r in slot r of `rsw` words at the misalignment of its place in HBM ---------------
template <int NL>
struct ScanStage {
  static constexpr int RSW = ((2 * WireStage<NL>::LMAX + 6) / 4 + 1) | 1;
  static constexpr int WORDS = (FP_BLOCK * RSW + 3) / 4 * 4;
};
// words of a slot: the aligned dwords an element touches at any misalignment, one more for the decoder's read past the
// value, odd so that the lanes' slots spread over the LDS banks.  scan_stage_in writes the dwords of the element only:
// the words behind them hold whatever the stage held, and the decoders mask what they read there.
__host__ __device__ inline u32 scan_row_words(size_t EB) { return (u32)((EB + 6) / 4 + 1) | 1u; }

// HBM -> LDS: row r = element tab[r] of `base` (SCAN_NONE: zeros).  Barriers on both sides.
__device__ __forceinline__ void scan_stage_in(u32* w, u32 rsw, const u32* tab, const uint8_t* base, size_t EB) {
  __syncthreads();
  const u32 nw = (u32)((EB + 6) / 4);
  const u32 dq = (u32)FP_BLOCK / nw, dr = (u32)FP_BLOCK % nw;
  u32 r = threadIdx.x / nw, i = threadIdx.x % nw;
  while (r < (u32)FP_BLOCK) {
    u32 v[4], pos[4];                                      // four loads in flight, then the four stores
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      u32 t = 0;
      pos[k] = SCAN_NONE;
      if (r < (u32)FP_BLOCK) {
        pos[k] = r * rsw + i;
        const u32 e = tab[r];
        if (e != SCAN_NONE) {
          const uint8_t* g = base + (size_t)e * EB;
          const u32 mis = (u32)((uintptr_t)g & 3u);
          if (i < (mis + (u32)EB + 3) / 4) t = ((const u32*)(g - mis))[i];
        }
      }
      v[k] = t;
      i += dr;
      r += dq;
      if (i >= nw) {
        i -= nw;
        ++r;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (pos[k] != SCAN_NONE) w[pos[k]] = v[k];
  }
  __syncthreads();
}

// LDS -> HBM: the rows the table names, each to its own place; a dword that is not wholly the row's goes byte by byte.
// Starts with a barrier.
__device__ __forceinline__ void scan_stage_out(const u32* w, u32 rsw, const u32* tab, uint8_t* base, size_t EB) {
  __syncthreads();
  const u32 nw = (u32)((EB + 6) / 4);
  const u32 dq = (u32)FP_BLOCK / nw, dr = (u32)FP_BLOCK % nw;
  u32 r = threadIdx.x / nw, i = threadIdx.x % nw;
  while (r < (u32)FP_BLOCK) {
    const u32 e = tab[r];
    if (e != SCAN_NONE) {
      uint8_t* g = base + (size_t)e * EB;
      const u32 mis = (u32)((uintptr_t)g & 3u);
      const u32 end = mis + (u32)EB, lo = 4 * i;
      if (lo < end) {
        if (lo >= mis && lo + 4 <= end) {
          ((u32*)(g - mis))[i] = w[r * rsw + i];
        } else {
          const uint8_t* sb = (const uint8_t*)(w + r * rsw);
          uint8_t* gb = g - mis;
          for (u32 b = lo; b < lo + 4; ++b)
            if (b >= mis && b < end) gb[b] = sb[b];
        }
      }
    }
    i += dr;
    r += dq;
    if (i >= nw) {
      i -= nw;
      ++r;
    }
  }
}

// Byte offset, inside the stage, of lane `tid`'s row when the row is element e of `base`.
__device__ __forceinline__ u32 scan_row_byte(u32 tid, u32 rsw, const uint8_t* base, u32 e, size_t EB) {
  return tid * rsw * 4u + (u32)((uintptr_t)(base + (size_t)e * EB) & 3u);
}

// The lane's result into its row of the stage, B = its first byte there.  Workgroup-uniform choice: the rows of an
// array at an even address start 0 or (L odd) 2 bytes into a dword, which the stream encoder serves.
template <int NL>
__device__ __forceinline__ void scan_encode(u32* w, u32 B, const uint8_t* base, int L, const Fp<NL>& x, const Fp<NL>& y) {
  const u32 a = (u32)((uintptr_t)base & 3u);
  if (StreamCodec<NL>::serves(L) && (a == 0 || (a == 2 && (L & 1)))) {
    limbs_to_wire_stream_at<NL>(w, B, L, x, y);
  } else {
    uint8_t* dst = (uint8_t*)w + B;
    limbs_to_wire<NL>(dst, L, x);
    limbs_to_wire<NL>(dst + L, L, y);
  }
}

// ---- level 1: the forward sweep's record and the backward sweep's row -------------------------------------------
// slot f (0: X, 1: Y, 2: Z, 3: the product of the Zs) of step j in the workspace
template <int NL>
__device__ __forceinline__ u32* scan_ws_slot(u32* ws, size_t wstride, u32 j, int f) {
  return ws + ((size_t)j * 4 + (size_t)f) * (size_t)NL * wstride;
}

// Prefix j of the lane after its addition: X, Y <18, Z <1 and Z_0 ... Z_j <2.  An identity prefix, a lane past its
// chunk's end and an accumulator whose Z vanished (the double of a point of order 2: the identity) take Z = 1.
template <int NL>
__device__ __forceinline__ void scan_g1_record(JacAcc<NL>& S, bool& acc_inf, bool live, u32* ws, size_t wstride, size_t lane,
                                               u32 j, LFp<NL>* L, const FpParams<NL>* __restrict__ P) {
  Fp<NL> z, t;
  a_load(z, S.Z);
  fp_reduce8(z, z, P);                      // <1 (Z <4)
  if (fp_is_zero_limbs(z)) acc_inf = true;
  fp_set(t, P->one);
  fp_select(z, acc_inf || !live, t, z);
  g_store<NL>(scan_ws_slot<NL>(ws, wstride, j, 2), wstride, lane, z);
  if (j) {
    g_load<NL>(t, scan_ws_slot<NL>(ws, wstride, j - 1, 3), wstride, lane);
    fp_mulv(z, t, z, P, L);                 // <2
  }
  g_store<NL>(scan_ws_slot<NL>(ws, wstride, j, 3), wstride, lane, z);
  fp_zero(z);
  a_load(t, S.X);
  fp_select(t, acc_inf, z, t);
  g_store<NL>(scan_ws_slot<NL>(ws, wstride, j, 0), wstride, lane, t);
  a_load(t, S.Y);
  fp_select(t, acc_inf, z, t);
  g_store<NL>(scan_ws_slot<NL>(ws, wstride, j, 1), wstride, lane, t);
}

// Prefix j as a plain canonical affine point (all zero: the identity).  inv (an AGPR slot) holds 1 / (Z_0 ... Z_j) on
// entry and 1 / (Z_0 ... Z_(j-1)) on exit; zs: an AGPR scratch slot.  Uses L[0], L[1].
template <int NL>
__device__ __forceinline__ void scan_g1_peel(Fp<NL>& x, Fp<NL>& y, AFp<NL>& inv, AFp<NL>& zs, u32* ws, size_t wstride, size_t lane,
                                             u32 j, LFp<NL>* L, const FpParams<NL>* __restrict__ P) {
  Fp<NL> r, u, zi;
  a_load(zi, inv);
  if (j) {
    g_load<NL>(r, scan_ws_slot<NL>(ws, wstride, j - 1, 3), wstride, lane);
    fp_mulv(u, zi, r, P, L);                // 1/Z_j <2   (4)
    a_store(zs, u);
    g_load<NL>(r, scan_ws_slot<NL>(ws, wstride, j, 2), wstride, lane);
    fp_mulv(u, zi, r, P, L);                // <2   (2)
    a_store(inv, u);
    a_load(zi, zs);
  }
  l_store(L + 1, zi);
  fp_sqr(u, L + 1, zi, P);                  // zi^2 <2
  g_load<NL>(r, scan_ws_slot<NL>(ws, wstride, j, 0), wstride, lane);
  fp_mulv(r, r, u, P, L);                   // x <2   (36)
  fp_mul(u, L + 1, u, P);                   // zi^3 <2
  fp_from_mont<NL>(x, r, P, L);
  g_load<NL>(r, scan_ws_slot<NL>(ws, wstride, j, 1), wstride, lane);
  fp_mulv(r, r, u, P, L);                   // y <2
  fp_from_mont<NL>(y, r, P, L);
}

}  // namespace bgn
