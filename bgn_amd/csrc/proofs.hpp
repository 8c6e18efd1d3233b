// proofs.hpp — the response of a proof of plaintext knowledge, arithmetic modulo the group order n (device function;
// compiles under the host emulation with the range checks).
//
// Replaces the big.Int lines of NewProofOfPlaintextKnowledge (gadgets.go:42-49):
//     DL = (r + c*v + R*z*c*(N/Key)) mod N  =  (nonce1 + c * (v + K*z)) mod n,   K = R*(n/q1) mod n folded once per key.
// n is odd and below p, so the Montgomery row product of fpmont.hpp runs unchanged over a second FpParams<NL> block
// whose modulus is n (engine.cpp builds it next to the block of p).  In this file "<B" after a value means "< B*n".
//
// What makes every bound below hold: fp_mul(a, b) returns (a*b + m*n)/R with m < R, which is < 2n whenever
// a*b < R*n.  With b a canonical constant (r2 = R^2 mod n < n) that is true of ANY a < R — any tight-limb value, in
// particular an operand the caller did not reduce (v, z, nonce1, K: whatever fits n_len bytes, and 8*n_len <=
// bits(n) + 7 < LIMB_BITS*NL) and a 256-bit challenge cut into pieces of NL limbs.  Between lazy values the rule of
// fpmont.hpp applies with n for p: B_a*B_b < 2^(LIMB_BITS*NL - bits(n)), at least 2^9.
//
// v, z, nonce1 and K are secrets: no branch and no address here depends on a value — the loops run over limb indices,
// the final reduction is a select.
#pragma once

#include "codec.hpp"

namespace bgn {

constexpr int POK_C_BYTES = 32;                                            // a sha256 digest
constexpr int POK_C_LIMBS = (8 * POK_C_BYTES + LIMB_BITS - 1) / LIMB_BITS;  // 9 limbs of 29 bits

// w*R mod n, lazy, for an integer w of any length given as CL tight limbs: the 256-bit challenge (CL = POK_C_LIMBS) and
// the over-long draw of randexp.hpp.  w = sum_k piece_k * R^k with pieces of NL limbs (R = 2^(LIMB_BITS*NL)): one piece
// when CL <= NL, three for the challenge at NL = 3; Horner over the pieces in Montgomery form, where a product by r2 is
// a product by R.  The bounds hold for any number of pieces: the accumulator is <4 going into a product and <2 out of it.
// (The pieces are taken by template recursion, from the top one down, not by a loop: with products of 36 limbs in its
// body a loop is not unrolled, and a run-time piece index would send c to scratch memory.)
template <int NL, int CL, int K>
__device__ __forceinline__ void wide_horner(Fp<NL>& acc, const Fp<CL>& c, const Fp<NL>& r2,
                                            const FpParams<NL>* __restrict__ N, LFp<NL>* stage) {
  constexpr int NPIECE = (CL + NL - 1) / NL;
  Fp<NL> piece, t;
#pragma unroll
  for (int j = 0; j < NL; ++j) piece.v[j] = (K * NL + j < CL) ? c.v[K * NL + j < CL ? K * NL + j : 0] : 0u;
  fp_mulv(t, piece, r2, N, stage);                 // piece < R, r2 < 1: piece*R <2
  if constexpr (K == NPIECE - 1) {
    acc = t;                                       // <2
  } else {
    fp_mulv(acc, acc, r2, N, stage);               // <4 * <1: acc*R <2
    fp_add(acc, acc, t);                           // <4
  }
  if constexpr (K > 0) wide_horner<NL, CL, K - 1>(acc, c, r2, N, stage);
}

template <int NL, int CL>
__device__ __forceinline__ void wide_to_mont(Fp<NL>& r, const Fp<CL>& c, const Fp<NL>& r2,
                                             const FpParams<NL>* __restrict__ N, LFp<NL>* stage) {
  wide_horner<NL, CL, (CL + NL - 1) / NL - 1>(r, c, r2, N, stage);      // <4 (<2 with one piece)
}

// dl = (nonce1 + c*(v + K*z)) mod n, canonical in [0, n).  v, z, a (= nonce1), K: tight limbs of any value below R.
template <int NL>
__device__ __forceinline__ void pok_response(Fp<NL>& dl, const Fp<NL>& v, const Fp<NL>& z, const Fp<NL>& a,
                                             const Fp<POK_C_LIMBS>& c, const Fp<NL>& K,
                                             const FpParams<NL>* __restrict__ N, LFp<NL>* stage) {
  Fp<NL> r2, cm, t, u;
  fp_set(r2, N->r2);                               // <1
  wide_to_mont<NL, POK_C_LIMBS>(cm, c, r2, N, stage);  // c*R <4
  fp_mulv(t, K, r2, N, stage);                     // K < R, r2 <1: K*R <2
  fp_mulv(u, z, r2, N, stage);                     // z*R <2
  fp_mulv(t, t, u, N, stage);                      // <2 * <2: K*z*R <2
  fp_mulv(u, v, r2, N, stage);                     // v*R <2
  fp_add(t, t, u);                                 // (v + K*z)*R <4
  fp_mulv(t, cm, t, N, stage);                     // <4 * <4: c*(v + K*z)*R <2
  fp_mulv(u, a, r2, N, stage);                     // nonce1*R <2
  fp_add(t, t, u);                                 // <4
  fp_from_mont<NL>(dl, t, N, stage);               // (t + m*n)/R <= n, then one select: [0, n)
}

// The same from the byte strings of the ABI: unsigned big-endian, v_len / z_len / a_len / k_len bytes (each at most
// n_len), the challenge POK_C_BYTES bytes; dl big-endian in n_len bytes at dst.
template <int NL>
__device__ __forceinline__ void pok_response_bytes(uint8_t* dst, int n_len, const uint8_t* v, int v_len, const uint8_t* z,
                                                   int z_len, const uint8_t* a, int a_len, const uint8_t* c,
                                                   const uint8_t* k, int k_len, const FpParams<NL>* __restrict__ N,
                                                   LFp<NL>* stage) {
  Fp<NL> vv, zz, aa, kk, dl;
  Fp<POK_C_LIMBS> cc;
  wire_to_limbs<NL>(vv, v, v_len);
  wire_to_limbs<NL>(zz, z, z_len);
  wire_to_limbs<NL>(aa, a, a_len);
  wire_to_limbs<NL>(kk, k, k_len);
  wire_to_limbs<POK_C_LIMBS>(cc, c, POK_C_BYTES);
  pok_response<NL>(dl, vv, zz, aa, cc, kk, N, stage);
  limbs_to_wire<NL>(dst, n_len, dl);
}

}  // namespace bgn
