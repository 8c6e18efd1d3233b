// emu_randexp.cpp — host emulation of the seeded expansion of blinding scalars (TEST INFRASTRUCTURE, built by
// tests/test_emu_randexp.py the way tests/test_emu_proofs.py builds its library): rand_block, rand_reduce and the whole
// scalar of csrc/randexp.hpp, the latter two with the range checks on.
#include <hip/hip_runtime.h>
#include <string.h>

thread_local int bgn_emu_checks = 0;
thread_local unsigned long long bgn_emu_tally[16] = {0};
struct EmuChecks { EmuChecks() { bgn_emu_checks = 1; } ~EmuChecks() { bgn_emu_checks = 0; } };
thread_local EmuDim3 threadIdx = {0, 0, 0}, blockIdx = {0, 0, 0}, gridDim = {1, 1, 1}, blockDim = {256, 1, 1};

#include "randexp.hpp"

using namespace bgn;

template <int NL>
static void reduce(const u32* params_n, const u32* w, u32* out) {
  static LFp<NL> stage;
  EmuChecks on;
  Fp<RandShape<NL>::WL> W;
  Fp<NL> r;
  for (int k = 0; k < RandShape<NL>::WL; ++k) W.v[k] = w[k];
  rand_reduce<NL>(r, W, (const FpParams<NL>*)params_n, &stage);
  for (int k = 0; k < NL; ++k) out[k] = r.v[k];
}

template <int NL>
static void scalar(const u32* params_n, int n_len, const u32 (&K)[RAND_SEED_WORDS], u64 t, u64 i, uint8_t* dst) {
  static LFp<NL> stage;
  EmuChecks on;
  rand_scalar_bytes<NL>(dst, n_len, K, t, i, (const FpParams<NL>*)params_n, &stage);
}

#define EACH_NL(X) X(3) X(10) X(19) X(36) X(37) X(72)

extern "C" {
// digest = B_j of (K, t, i): 32 bytes; K as eight big-endian words
void randexp_block(const u32* k8, unsigned long long t, unsigned long long i, unsigned j, uint8_t* digest) {
  u32 K[RAND_SEED_WORDS], st[8];
  for (int m = 0; m < RAND_SEED_WORDS; ++m) K[m] = k8[m];
  rand_block(K, t, i, j, st);
  sha256_store(digest, st);
}

// limbs of the longest W and the longest group order of an instantiation; -1: unknown limb count
int randexp_w_limbs(int nl) {
  switch (nl) {
#define X(N) case N: return RandShape<N>::WL;
    EACH_NL(X)
#undef X
    default: return -1;
  }
}
int randexp_max_n_len(int nl) {
  switch (nl) {
#define X(N) case N: return RandShape<N>::MAX_N_LEN;
    EACH_NL(X)
#undef X
    default: return -1;
  }
}

// out (nl limbs) = W mod n for W given as randexp_w_limbs(nl) tight limbs (a failed range check aborts with its message)
int randexp_reduce(int nl, const u32* params_n, const u32* w, u32* out) {
  switch (nl) {
#define X(N) case N: reduce<N>(params_n, w, out); break;
    EACH_NL(X)
#undef X
    default: return -1;
  }
  return 0;
}

// dst (n_len bytes) = the scalar of (K, t, i)
int randexp_scalar(int nl, const u32* params_n, int n_len, const u32* k8, unsigned long long t, unsigned long long i,
                   uint8_t* dst) {
  u32 K[RAND_SEED_WORDS];
  for (int m = 0; m < RAND_SEED_WORDS; ++m) K[m] = k8[m];
  switch (nl) {
#define X(N) case N: scalar<N>(params_n, n_len, K, t, i, dst); break;
    EACH_NL(X)
#undef X
    default: return -1;
  }
  return 0;
}
}
