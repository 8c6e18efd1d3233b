// compressops.hpp — the compressed wire form (include/bgn_amd.h: L + 1 bytes, the abscissa resp. the real part and one
// flag byte) on the device: k_compress_wire and k_decompress.
//
// k_compress_wire is k_neg_wire's class: stage the slice, decode x, look at one bit of y, encode, write — no field
// product, one WireStage of LDS, nothing else.  Level 1 reads y's last byte out of the stage and never decodes it;
// level 2 decodes im because a residue >= p must be reduced before its parity means anything (rare: checked per wave).
// A compressed element is L + 1 bytes, so element e starts at any byte of a dword, another one on every lane:
// cz_encode cuts the aligned words of the lane's element out of the little-endian dwords of V = flag + x * 2^8 with
// one v_perm_b32 each, as the stream codec does, with the byte shift per lane, and writes the up to three bytes in
// front of the first aligned word and behind the last one as bytes — no lane touches a word it shares.
//
// k_decompress, one element per lane: x and the flag out of the odd-sized stream, rhs = x^3 + x (level 1) or
// 1 - re^2 (level 2) in Montgomery form, root = rhs^((p+1)/4), root^2 == rhs, the root of the flag's parity, the
// rejection rules, both coordinates encoded.  The exponent is the key's: sqrtrecode.hpp turns it into a program of
// (squarings, odd power) ops once per context, read here through a wave-uniform pointer — every lane of every wave
// runs the same squarings and the same products, no digit is fetched per lane and nothing diverges.
//
// The windows.  A width-w table is 2^(w-1) odd powers of NL limbs per lane; beside the squaring's working set (2 NL
// accumulator registers and NL for the operand) it does not fit the 256 VGPRs.  Two places can hold it:
//   (a) narrow windows, the powers in AGPR slots: w = 3, four powers (148 AGPRs at 37 limbs, a fifth slot keeps x).
//       For a 1030-bit exponent: ~1027 squarings + ~260 products + 1 + 3 for the table.  A power reaches the product
//       through a wave-uniform branch, 36 v_accvgpr_read and 18 LDS writes: 2 % of the product behind them.
//   (b) w = 5, sixteen powers limb-major in the workspace, as the pairing's window tables: ~1025 squarings + ~172
//       products + 1 + 15 for the table, and 2.3 KB of HBM per element written once and gathered ~172 times.
// Priced with a product at 1.2 squarings (8.0 against 6.6 us per wave, fpmont.hpp): (a) 1344, (b) 1251 squarings'
// worth — (b) is 7 % less arithmetic for a workspace of 2.4 GB per 2^20 elements.  (a) is built.  (w = 4 needs eight
// slots and x: 333 AGPRs.)
// Multiply-adds per element at NL limbs: a squaring is NL^2 (reduction) + ~0.6 NL^2 (five segments), a product 2 NL^2;
// 36 limbs: 1028 * 2074 + 263 * 2592 = 2.8 x 10^6.
#pragma once
#include "codec.hpp"
#include "scanops.hpp"

namespace bgn {

// a < p  <=>  a - p borrows
template <int NL>
__device__ __forceinline__ bool cz_lt_p(const Fp<NL>& a, const FpParams<NL>* __restrict__ P) {
  i32 c = 0;
#pragma unroll
  for (int j = 0; j < NL; ++j) c = ((i32)a.v[j] - (i32)P->p[j] + c) >> LIMB_BITS;
  return c != 0;
}

// The canonical residue of a value read from L wire bytes: it is below 2^(8L) <= 256 p, so eight conditional
// subtractions of 32 p leave it below 32 p and five more passes below p.  No product and no LDS slot: the kernel keeps
// k_neg_wire's footprint.  Runs only in a wave that holds a residue >= p.
template <int NL>
__device__ __forceinline__ void cz_canon(Fp<NL>& a, const FpParams<NL>* __restrict__ P) {
#pragma unroll 1
  for (int k = 0; k < 8; ++k) {
    Fp<NL> d;
    i32 c = 0;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const i32 v = (i32)a.v[j] - (i32)P->kp[KP_MAX - 1][j] + c;
      d.v[j] = (u32)v & LIMB_MASK;
      c = v >> LIMB_BITS;
    }
    fp_select(a, c == 0, d, a);
  }
  fp_reduce_lt<NL, 32>(a, a, P);
}

// The big-endian L-byte value at byte B (any alignment, per lane) of the stage.
template <int NL>
__device__ __forceinline__ void cz_value(Fp<NL>& r, const u32* __restrict__ w, u32 B, int L) {
  if (StreamCodec<NL>::serves(L))                          // wave-uniform
    wire_to_limbs_stream<NL>(r, w, B, L);
  else
    wire_to_limbs<NL>(r, (const uint8_t*)w + B, L);
}

// x (canonical) big-endian in L bytes, then the flag byte, into the L + 1 bytes at byte B of the stage; B is any byte
// address and differs from lane to lane.  Read backwards the element is the little-endian number V = flag + x * 2^8.
// With r = (B + L + 1) & 3 bytes of the element in its last, partial word, the aligned word i below that one is the
// big-endian 32-bit number at byte 4i + r of V: one v_perm_b32 of V's dwords i and i + 1 (register indices at compile
// time, the byte shift r in the selector, per lane), stored while the word lies inside the element (per lane: lanes
// differ by one word).  The r bytes behind are V's lowest, the (-B) & 3 bytes in front its highest: byte stores.
template <int NL>
__device__ __forceinline__ void cz_encode(u32* __restrict__ w, u32 B, int L, const Fp<NL>& x, u32 flag) {
  uint8_t* wb = (uint8_t*)w;
  if (!StreamCodec<NL>::serves(L)) {                       // wave-uniform
    limbs_to_wire<NL>(wb + B, L, x);
    wb[B + (u32)L] = (uint8_t)flag;
    return;
  }
  constexpr int ND = StreamCodec<NL>::ND, FMIN = StreamCodec<NL>::FMIN;
  u32 vd[ND + 2];
  u32 prev = flag & 0xFFu;
#pragma unroll
  for (int i = 0; i < ND; ++i) {
    const u32 xd = limbs_dword<NL>(x, i);
    vd[i] = (xd << 8) | prev;
    prev = xd >> 24;
  }
  vd[ND] = prev;
  vd[ND + 1] = 0;
  const u32 CL = (u32)L + 1u;
  const u32 end = B + CL;
  const u32 r = end & 3u, qe = end >> 2;
  const u32 sel = stream_sel(r);
#pragma unroll
  for (int i = 0; i <= ND; ++i)
    if (4u * (u32)i + r + 4u <= CL) w[qe - 1u - (u32)i] = codec_perm(vd[i + 1], vd[i], sel);
  // V's top four bytes (bytes L - 3 .. L): dword index and shift are wave-uniform, the register index is not allowed
  // to be — a chain of selects over the few dwords it can be
  const int ti = (L - 3) >> 2;
  const u32 tb = 8u * (u32)((L - 3) & 3);
  u32 top4 = 0;
#pragma unroll
  for (int i = (FMIN > 0 ? FMIN - 1 : 0); i <= ND; ++i) top4 = (i == ti) ? codec_funnel(vd[i + 1], vd[i], tb) : top4;
  const u32 h = (0u - B) & 3u;
#pragma unroll
  for (u32 s = 0; s < 3; ++s)
    if (s < h) wb[B + s] = (uint8_t)(top4 >> (8u * (3u - s)));
#pragma unroll
  for (u32 k = 0; k < 3; ++k)
    if (k < r) wb[4u * qe + k] = (uint8_t)(vd[0] >> ((8u * (r - 1u - k)) & 31u));
}

// Full form -> compressed form, wire bytes to wire bytes in one launch; both arrays at any byte address.
template <int NL>
__global__ void __launch_bounds__(FP_BLOCK)
k_compress_wire(const FpParams<NL>* __restrict__ P, const uint8_t* __restrict__ in, int L, size_t count, int level,
                uint8_t* __restrict__ out) {
  __shared__ WireStage<NL> ws;
  const size_t e0 = (size_t)blockIdx.x * FP_BLOCK;
  const size_t nel = (count - e0 < (size_t)FP_BLOCK) ? count - e0 : (size_t)FP_BLOCK;
  const size_t EB = (size_t)(2 * L), CL = (size_t)L + 1;
  const bool live = threadIdx.x < nel;
  Fp<NL> x;
  u32 flag;
  {
    const u32 mis = wire_stage_in<NL>(&ws, in + e0 * EB, nel * EB);
    const u32 B = mis + (live ? threadIdx.x * (u32)EB : 0u);          // idle lanes decode element 0: discarded
    cz_value<NL>(x, ws.w, B, L);
    if (level == 1) {                                                  // wave-uniform
      // the identity is all zero; no finite point but (0, 0), which shares its bytes, has x = 0
      const u32 ylow = ((const uint8_t*)ws.w)[B + (u32)EB - 1u];
      flag = fp_is_zero_limbs(x) ? 0u : (2u | (ylow & 1u));
    } else {
      Fp<NL> y;
      cz_value<NL>(y, ws.w, B + (u32)L, L);
      if (__ballot(!(cz_lt_p<NL>(x, P) && cz_lt_p<NL>(y, P)))) {
        cz_canon<NL>(x, P);
        cz_canon<NL>(y, P);
      }
      flag = 2u | (y.v[0] & 1u);
    }
  }
  __syncthreads();                        // every lane has read its element: the stage takes the results
  uint8_t* g = out + e0 * CL;
  if (live) cz_encode<NL>(ws.w, (u32)((uintptr_t)g & 3u) + threadIdx.x * (u32)CL, L, x, flag);
  wire_stage_out<NL>(&ws, g, nel * CL);
}

// the odd power `idx` (wave-uniform) out of its AGPR slot: registers cannot be indexed at run time
template <int NL>
__device__ __forceinline__ void cz_pick(Fp<NL>& r, u32 idx, const AFp<NL>& T0, const AFp<NL>& T1, const AFp<NL>& T2,
                                        const AFp<NL>& T3) {
  if (idx == 0)
    a_load(r, T0);
  else if (idx == 1)
    a_load(r, T1);
  else if (idx == 2)
    a_load(r, T2);
  else
    a_load(r, T3);
}

// Compressed form -> full canonical wire bytes and ok[e]; both arrays at any byte address.  ops / nops: the program of
// sqrtrecode.hpp for (p + 1) / 4.  LDS: two product slots and the stage (k_g1_add_wire's footprint).
template <int NL>
__global__ void __launch_bounds__(FP_BLOCK)
k_decompress(const FpParams<NL>* __restrict__ P, const uint16_t* __restrict__ ops, int nops,
             const uint8_t* __restrict__ in, int L, size_t count, int level, uint8_t* __restrict__ out,
             uint8_t* __restrict__ ok) {
  __shared__ LFp<NL> Ls[2];
  __shared__ WireStage<NL> ws;
  const size_t e0 = (size_t)blockIdx.x * FP_BLOCK;
  const size_t nel = (count - e0 < (size_t)FP_BLOCK) ? count - e0 : (size_t)FP_BLOCK;
  const size_t EB = (size_t)(2 * L), CL = (size_t)L + 1;
  const bool live = threadIdx.x < nel;
  AFp<NL> SX, T0, T1, T2, T3;
  Fp<NL> a, t, acc;
  u32 flag;
  bool good, xz;
  {
    const u32 mis = wire_stage_in<NL>(&ws, in + e0 * CL, nel * CL);
    const u32 B = mis + (live ? threadIdx.x * (u32)CL : 0u);          // idle lanes decode element 0: discarded
    cz_value<NL>(a, ws.w, B, L);
    flag = ((const uint8_t*)ws.w)[B + (u32)L];
    good = cz_lt_p<NL>(a, P);
    xz = fp_is_zero_limbs(a);
    a_store(SX, a);
  }
  __syncthreads();                        // every lane has read its element: the stage is free for the results
  fp_to_mont<NL>(a, a, P, Ls);            // <1 (the product takes an x >= p too; its lane is rejected already)
  fp_sqrv(t, a, P, Ls);                   // x^2 <2
  if (level == 1) {                       // wave-uniform
    fp_mulv(t, t, a, P, Ls);              // x^3 <2
    fp_add(a, t, a);                      // rhs = x^3 + x <3
  } else {
    fp_set(acc, P->one);
    fp_sub<2>(a, acc, t, P);              // rhs = 1 - re^2 <3
  }
  a_store(T0, a);
  fp_sqrv(t, a, P, Ls);                   // rhs^2 <2
  l_store(Ls + 1, t);
  fp_mul(a, Ls + 1, a, P);                // rhs^3 <2   (6)
  a_store(T1, a);
  fp_mul(a, Ls + 1, a, P);                // rhs^5 <2   (4)
  a_store(T2, a);
  fp_mul(a, Ls + 1, a, P);                // rhs^7 <2
  a_store(T3, a);
  cz_pick<NL>(acc, (u32)ops[0] >> 8, T0, T1, T2, T3);
#pragma unroll 1
  for (int o = 1; o < nops; ++o) {
    const u32 op = ops[o];
#pragma unroll 1
    for (u32 s = op & 0xFFu; s; --s) fp_sqrv(acc, acc, P, Ls);        // <2
    if ((op >> 8) != 0xFFu) {
      cz_pick<NL>(t, op >> 8, T0, T1, T2, T3);
      l_store(Ls + 1, t);
      fp_mul(acc, Ls + 1, acc, P);                                    // <2   (6)
    }
  }
  // root^2 == rhs ?
  fp_sqrv(t, acc, P, Ls);                 // <2
  a_load(a, T0);
  fp_sub<3>(t, t, a, P);                  // <5
  fp_from_mont<NL>(a, t, P, Ls);          // canonical: zero iff rhs is a square (or zero)
  good = good && fp_is_zero_limbs(a);
  Fp<NL> y;
  fp_from_mont<NL>(y, acc, P, Ls);        // the root, canonical
  const bool yz = fp_is_zero_limbs(y);
  fp_neg<1>(t, y, P);                     // p - y: the other root (y = 0 has none; flag 0x03 is then refused)
  fp_select(y, ((y.v[0] ^ flag) & 1u) != 0, t, y);
  const bool finite = flag == 2u || flag == 3u;
  good = good && finite && !(yz && flag == 3u);
  bool ident = false;
  if (level == 1) {
    ident = flag == 0u && xz;             // the one spelling of the identity
    good = good && !xz;                   // (0, 0) has the identity's full-form bytes: 0 || 0x02 is refused
  }
  a_load(a, SX);
  fp_zero(t);
  fp_select(y, good, y, t);
  if (level == 2) t.v[0] = 1;             // level 2's identity is 1 || 0
  fp_select(a, good, a, t);
  uint8_t* g = out + e0 * EB;
  if (live) scan_encode<NL>(ws.w, (u32)((uintptr_t)g & 3u) + threadIdx.x * (u32)EB, g, L, a, y);
  wire_stage_out<NL>(&ws, g, nel * EB);
  if (live) ok[e0 + threadIdx.x] = (good || ident) ? 1 : 0;
}

}  // namespace bgn
