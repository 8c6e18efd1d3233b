// sha256.hpp — SHA-256 (FIPS 180-4) of two wire elements, one message per lane (device function; compiles under the
// host emulation).
//
// Replaces hash() of the reference (gadgets.go:80-96): the Fiat-Shamir challenge of a proof of plaintext knowledge is
// sha256(proof.Ct.C.Bytes() || proof.Nonce.C.Bytes()) read as a big-endian integer.  Both operands are device
// arrays of 2L bytes per element at ANY byte address (2L = 2 mod 4 at L = 129, and the ABI lets an array start
// anywhere), so the message words are cut out of aligned dwords with one v_perm_b32 whose selector carries the lane's
// misalignment; the few words that straddle the seam between the operands, the 0x80 marker or the length field are
// put together byte by byte.
//
// Registers: the message schedule is a rolling window of 16 words and the eight state words rotate by renaming — the
// 64 rounds are written out, every index is a literal, nothing is indexed at run time (a run-time index into w[] would
// send it to scratch memory).  The block loop is the only loop; its trip count follows from the length, a kernel
// argument.
#pragma once

#include "codec.hpp"

namespace bgn {

__device__ __forceinline__ u32 sha_rotr(u32 x, int n) { return (x >> n) | (x << (32 - n)); }
__device__ __forceinline__ u32 sha_S0(u32 x) { return sha_rotr(x, 2) ^ sha_rotr(x, 13) ^ sha_rotr(x, 22); }
__device__ __forceinline__ u32 sha_S1(u32 x) { return sha_rotr(x, 6) ^ sha_rotr(x, 11) ^ sha_rotr(x, 25); }
__device__ __forceinline__ u32 sha_s0(u32 x) { return sha_rotr(x, 7) ^ sha_rotr(x, 18) ^ (x >> 3); }
__device__ __forceinline__ u32 sha_s1(u32 x) { return sha_rotr(x, 17) ^ sha_rotr(x, 19) ^ (x >> 10); }
__device__ __forceinline__ u32 sha_ch(u32 e, u32 f, u32 g) { return g ^ (e & (f ^ g)); }
__device__ __forceinline__ u32 sha_maj(u32 a, u32 b, u32 c) { return (a & b) | (c & (a | b)); }

// The big-endian 32-bit number at p (any alignment; all four bytes inside the array): the aligned dword that holds
// p[0] and, when p is not aligned, the next one — no dword is read that holds no byte of the number.
__device__ __forceinline__ u32 sha_be_word(const uint8_t* p) {
  const uintptr_t ad = (uintptr_t)p;
  const u32 mis = (u32)(ad & 3u);
  const u32* q = (const u32*)(ad - mis);
  const u32 w0 = q[0];
  const u32 w1 = mis ? q[1] : 0u;
  return codec_perm(w1, w0, stream_sel(mis));
}

// Byte m of the padded message a || b || 0x80 || 0.. || bit length (64 bits, big-endian), `padded` bytes in all.
__device__ __forceinline__ u32 sha_msg_byte(const uint8_t* a, const uint8_t* b, size_t len, size_t padded, size_t m) {
  if (m < len) return a[m];
  if (m < 2 * len) return b[m - len];
  if (m == 2 * len) return 0x80u;
  if (m + 8 >= padded) {
    const unsigned long long bits = (unsigned long long)(2 * len) * 8u;
    return (u32)(bits >> (8 * (padded - 1 - m))) & 0xFFu;
  }
  return 0u;
}

// Word j of the padded message.  The position is the same on every lane (the length is a kernel argument), so the
// choice between the three forms is wave-uniform; what differs per lane is the alignment, which is data.
__device__ __forceinline__ u32 sha_msg_word(const uint8_t* a, const uint8_t* b, size_t len, size_t padded, size_t j) {
  const size_t off = 4 * j;
  if (off + 4 <= len) return sha_be_word(a + off);
  if (off >= len && off + 4 <= 2 * len) return sha_be_word(b + (off - len));
  u32 w = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) w = (w << 8) | sha_msg_byte(a, b, len, padded, off + (size_t)i);
  return w;
}

#define BGN_SHA_RND(a, b, c, d, e, f, g, h, t, k)                                                              \
  do {                                                                                                         \
    u32 wt;                                                                                                    \
    if ((t) < 16) {                                                                                            \
      wt = w[(t) & 15];                                                                                        \
    } else {                                                                                                   \
      wt = w[(t) & 15] + sha_s1(w[((t) - 2) & 15]) + w[((t) - 7) & 15] + sha_s0(w[((t) - 15) & 15]);           \
      w[(t) & 15] = wt;                                                                                        \
    }                                                                                                          \
    const u32 t1 = (h) + sha_S1(e) + sha_ch(e, f, g) + (k) + wt;                                               \
    const u32 t2 = sha_S0(a) + sha_maj(a, b, c);                                                               \
    (d) += t1;                                                                                                 \
    (h) = t1 + t2;                                                                                             \
  } while (0)

// eight rounds: the state words come back to their own names
#define BGN_SHA_RND8(t, k0, k1, k2, k3, k4, k5, k6, k7)    \
  BGN_SHA_RND(a, b, c, d, e, f, g, h, (t) + 0, k0);        \
  BGN_SHA_RND(h, a, b, c, d, e, f, g, (t) + 1, k1);        \
  BGN_SHA_RND(g, h, a, b, c, d, e, f, (t) + 2, k2);        \
  BGN_SHA_RND(f, g, h, a, b, c, d, e, (t) + 3, k3);        \
  BGN_SHA_RND(e, f, g, h, a, b, c, d, (t) + 4, k4);        \
  BGN_SHA_RND(d, e, f, g, h, a, b, c, (t) + 5, k5);        \
  BGN_SHA_RND(c, d, e, f, g, h, a, b, (t) + 6, k6);        \
  BGN_SHA_RND(b, c, d, e, f, g, h, a, (t) + 7, k7)

// the 64 rounds of one compression over w[16] and a..h (FIPS 180-4 section 4.2.2 constants)
#define BGN_SHA_ROUNDS64()                                                                                             \
  BGN_SHA_RND8(0, 0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u); \
  BGN_SHA_RND8(8, 0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u); \
  BGN_SHA_RND8(16, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau); \
  BGN_SHA_RND8(24, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u); \
  BGN_SHA_RND8(32, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u); \
  BGN_SHA_RND8(40, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u); \
  BGN_SHA_RND8(48, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u); \
  BGN_SHA_RND8(56, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u)

// out[0..8) = the state words of sha256(pa[0..len_each) || pb[0..len_each)): the digest is their big-endian bytes in
// order.  Reads only bytes of the two arrays (through the aligned dwords that hold them).
__device__ __forceinline__ void sha256_wire(const uint8_t* pa, const uint8_t* pb, size_t len_each, u32 out[8]) {
  const size_t nblk = (2 * len_each + 9 + 63) / 64;       // 0x80 and the 8-byte length always fit the last block
  const size_t padded = 64 * nblk;
  u32 h0 = 0x6a09e667u, h1 = 0xbb67ae85u, h2 = 0x3c6ef372u, h3 = 0xa54ff53au;
  u32 h4 = 0x510e527fu, h5 = 0x9b05688cu, h6 = 0x1f83d9abu, h7 = 0x5be0cd19u;
#pragma unroll 1
  for (size_t blk = 0; blk < nblk; ++blk) {
    u32 w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = sha_msg_word(pa, pb, len_each, padded, 16 * blk + (size_t)i);
    u32 a = h0, b = h1, c = h2, d = h3, e = h4, f = h5, g = h6, h = h7;
    BGN_SHA_ROUNDS64();
    h0 += a; h1 += b; h2 += c; h3 += d; h4 += e; h5 += f; h6 += g; h7 += h;
  }
  out[0] = h0; out[1] = h1; out[2] = h2; out[3] = h3; out[4] = h4; out[5] = h5; out[6] = h6; out[7] = h7;
}

// The digest bytes of `st` at dst (any alignment).
__device__ __forceinline__ void sha256_store(uint8_t* dst, const u32 st[8]) {
  if (((uintptr_t)dst & 3u) == 0) {
    u32* d4 = (u32*)dst;
#pragma unroll
    for (int i = 0; i < 8; ++i) d4[i] = codec_perm(0, st[i], 0x00010203u);
  } else {
#pragma unroll
    for (int i = 0; i < 32; ++i) dst[i] = (uint8_t)(st[i >> 2] >> (8 * (3 - (i & 3))));
  }
}

}  // namespace bgn
