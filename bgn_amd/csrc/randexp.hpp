// randexp.hpp — blinding scalars expanded from a caller's 32-byte seed, "expansion 1" of include/bgn_amd.h (device
// functions; compile under the host emulation with the range checks).
//
// Replaces newCryptoRandom(N) of the reference (bgn.go:567-574) behind Encrypt (bgn.go:334-337) for callers that keep a
// chain on the device: the engine still draws nothing — for seed K, stream id t and element index i
//     B_j = SHA-256(K || be64(t) || be64(i) || be32(j))             52 bytes: one compression per block
//     W   = the first n_len + 16 bytes of B_0 || B_1 || ...,        a big-endian integer
//     r   = W mod n,  n_len big-endian bytes                        16 surplus bytes: bias below 2^-128
// The message words come from kernel arguments and the lane's index — nothing is read from memory, and the seed is
// never written to any.  n_len is a kernel argument (public, wave-uniform): the loop over the blocks and the shifts
// that cut W out of them branch on it alone.  r is a secret: no branch and no address depends on a block word or on
// anything computed from one — W is cut with shifts by wave-uniform amounts, every array index is a literal after
// unrolling (a run-time index would send the words to scratch memory), and W mod n is wide_to_mont (proofs.hpp) with
// the one select of fp_from_mont at the end.
#pragma once

#include "sha256.hpp"
#include "proofs.hpp"

namespace bgn {

constexpr int RAND_SEED_WORDS = 8;       // K as big-endian 32-bit words
constexpr int RAND_SURPLUS_BYTES = 16;   // bytes of W beyond n_len
constexpr int RAND_BLOCK_BYTES = 32;     // a sha256 digest

// What an instantiation must hold for every key it serves.  The engine picks NL with bits(p) + 9 <= LIMB_BITS*NL and
// n < p, so 8*n_len <= bits(n) + 7 <= LIMB_BITS*NL - 2.
template <int NL>
struct RandShape {
  static constexpr int MAX_N_LEN = (LIMB_BITS * NL - 2) / 8;
  static constexpr int MAX_W_LEN = MAX_N_LEN + RAND_SURPLUS_BYTES;
  static constexpr int NBLK = (MAX_W_LEN + RAND_BLOCK_BYTES - 1) / RAND_BLOCK_BYTES;
  static constexpr int NW = 8 * NBLK;                                           // 32-bit words of all the blocks
  static constexpr int WL = (8 * MAX_W_LEN + LIMB_BITS - 1) / LIMB_BITS;        // limbs of the longest W
};

// out[0..8) = the state words of B_j: one compression of the padded 52-byte message.  Words 0-9 (K, t) and 12-15 (j,
// the 0x80 marker, the bit length 416) are the same on every lane; words 10 and 11 are the lane's index.  The message
// has a fixed length, so its padding is a constant and no message is a prefix of another.
__device__ __forceinline__ void rand_block(const u32 (&K)[RAND_SEED_WORDS], u64 t, u64 i, u32 j, u32 out[8]) {
  u32 w[16];
#pragma unroll
  for (int m = 0; m < RAND_SEED_WORDS; ++m) w[m] = K[m];
  w[8] = (u32)(t >> 32);
  w[9] = (u32)t;
  w[10] = (u32)(i >> 32);
  w[11] = (u32)i;
  w[12] = j;
  w[13] = 0x80000000u;
  w[14] = 0u;
  w[15] = 8u * 52u;
  const u32 h0 = 0x6a09e667u, h1 = 0xbb67ae85u, h2 = 0x3c6ef372u, h3 = 0xa54ff53au;
  const u32 h4 = 0x510e527fu, h5 = 0x9b05688cu, h6 = 0x1f83d9abu, h7 = 0x5be0cd19u;
  u32 a = h0, b = h1, c = h2, d = h3, e = h4, f = h5, g = h6, h = h7;
  BGN_SHA_ROUNDS64();
  out[0] = h0 + a; out[1] = h1 + b; out[2] = h2 + c; out[3] = h3 + d;
  out[4] = h4 + e; out[5] = h5 + f; out[6] = h6 + g; out[7] = h7 + h;
}

// W of (K, t, i) for a group order of n_len bytes (at most RandShape<NL>::MAX_N_LEN), as tight limbs.
// x[] holds the blocks drawn so far as one integer, lowest word first: a new block moves the others up by eight words
// and takes the bottom, so after the last one B_0 is on top and 32*nblk - wlen surplus bytes (0..31) hang off the low
// end; a word shift in three conditional steps and one funnel shift by bytes drop them.
template <int NL>
__device__ __forceinline__ void rand_draw(Fp<RandShape<NL>::WL>& W, const u32 (&K)[RAND_SEED_WORDS], u64 t, u64 i, int n_len) {
  constexpr int NW = RandShape<NL>::NW, WL = RandShape<NL>::WL;
  const int wlen = n_len + RAND_SURPLUS_BYTES;
  const int nblk = (wlen + RAND_BLOCK_BYTES - 1) / RAND_BLOCK_BYTES;
  BGN_CHECK_ALWAYS(n_len >= 1 && nblk <= RandShape<NL>::NBLK, "rand_draw: group order longer than the instantiation serves");
  u32 x[NW];
#pragma unroll
  for (int m = 0; m < NW; ++m) x[m] = 0u;
#pragma unroll 1
  for (int j = 0; j < nblk; ++j) {
    u32 blk[8];
    rand_block(K, t, i, (u32)j, blk);
#pragma unroll
    for (int m = NW - 1; m >= 8; --m) x[m] = x[m - 8];
#pragma unroll
    for (int m = 0; m < 8; ++m) x[m] = blk[7 - m];
  }
  const int drop = RAND_BLOCK_BYTES * nblk - wlen;          // wave-uniform, 0..31
#pragma unroll
  for (int s = 4; s >= 1; s >>= 1) {
    if ((drop >> 2) & s) {
#pragma unroll
      for (int m = 0; m < NW; ++m) x[m] = (m + s < NW) ? x[m + s < NW ? m + s : 0] : 0u;
    }
  }
  const int bs = 8 * (drop & 3);
#pragma unroll
  for (int m = 0; m < NW; ++m) {
    const u32 hi = (m + 1 < NW) ? x[m + 1 < NW ? m + 1 : 0] : 0u;
    x[m] = (u32)((((u64)hi << 32) | x[m]) >> bs);
  }
#pragma unroll
  for (int k = 0; k < WL; ++k) {
    const int m = (LIMB_BITS * k) >> 5, o = (LIMB_BITS * k) & 31;
    u32 v = (m < NW) ? x[m < NW ? m : 0] >> o : 0u;
    if (o + LIMB_BITS > 32 && m + 1 < NW) v |= x[m + 1 < NW ? m + 1 : 0] << ((32 - o) & 31);
    W.v[k] = v & LIMB_MASK;
  }
}

// r = W mod n, canonical in [0, n), over the parameter block of n.
template <int NL>
__device__ __forceinline__ void rand_reduce(Fp<NL>& r, const Fp<RandShape<NL>::WL>& W, const FpParams<NL>* __restrict__ N,
                                            LFp<NL>* stage) {
  Fp<NL> r2, wm;
  fp_set(r2, N->r2);                                             // <1
  wide_to_mont<NL, RandShape<NL>::WL>(wm, W, r2, N, stage);      // W*R <4
  fp_from_mont<NL>(r, wm, N, stage);                             // (wm + m*n)/R <= n, then one select: [0, n)
}

// The scalar of (K, t, i) as n_len big-endian bytes at dst (any alignment).
template <int NL>
__device__ __forceinline__ void rand_scalar_bytes(uint8_t* dst, int n_len, const u32 (&K)[RAND_SEED_WORDS], u64 t, u64 i,
                                                  const FpParams<NL>* __restrict__ N, LFp<NL>* stage) {
  Fp<RandShape<NL>::WL> W;
  Fp<NL> r;
  rand_draw<NL>(W, K, t, i, n_len);
  rand_reduce<NL>(r, W, N, stage);
  limbs_to_wire<NL>(dst, n_len, r);
}

}  // namespace bgn
