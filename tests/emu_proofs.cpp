// emu_proofs.cpp — host emulation of the two device functions behind the proofs of plaintext knowledge (TEST
// INFRASTRUCTURE, built by tests/test_emu_proofs.py the way tests/test_emu_curve_a3.py builds its library):
// sha256_wire of sha256.hpp and pok_response_bytes of proofs.hpp, the latter with the range checks on.
#include <hip/hip_runtime.h>
#include <string.h>

thread_local int bgn_emu_checks = 0;
thread_local unsigned long long bgn_emu_tally[16] = {0};
struct EmuChecks { EmuChecks() { bgn_emu_checks = 1; } ~EmuChecks() { bgn_emu_checks = 0; } };
thread_local EmuDim3 threadIdx = {0, 0, 0}, blockIdx = {0, 0, 0}, gridDim = {1, 1, 1}, blockDim = {256, 1, 1};

#include "sha256.hpp"
#include "proofs.hpp"

using namespace bgn;

template <int NL>
static void response(const u32* params_n, int n_len, const uint8_t* v, int v_len, const uint8_t* z, int z_len, const uint8_t* a,
                     int a_len, const uint8_t* c, const uint8_t* k, int k_len, uint8_t* dl) {
  static LFp<NL> stage;
  EmuChecks on;
  pok_response_bytes<NL>(dl, n_len, v, v_len, z, z_len, a, a_len, c, k, k_len, (const FpParams<NL>*)params_n, &stage);
}

extern "C" {
// digest = sha256(a[0..len) || b[0..len)), 32 bytes
void proofs_sha256_wire(const uint8_t* a, const uint8_t* b, size_t len_each, uint8_t* digest) {
  u32 st[8];
  sha256_wire(a, b, len_each, st);
  sha256_store(digest, st);
}

// one response over the parameter block of n (a failed range check aborts with its message); -1: unknown limb count
int proofs_response(int nl, const u32* params_n, int n_len, const uint8_t* v, int v_len, const uint8_t* z, int z_len,
                    const uint8_t* a, int a_len, const uint8_t* c, const uint8_t* k, int k_len, uint8_t* dl) {
  switch (nl) {
    case 3: response<3>(params_n, n_len, v, v_len, z, z_len, a, a_len, c, k, k_len, dl); break;
    case 10: response<10>(params_n, n_len, v, v_len, z, z_len, a, a_len, c, k, k_len, dl); break;
    case 19: response<19>(params_n, n_len, v, v_len, z, z_len, a, a_len, c, k, k_len, dl); break;
    case 36: response<36>(params_n, n_len, v, v_len, z, z_len, a, a_len, c, k, k_len, dl); break;
    case 37: response<37>(params_n, n_len, v, v_len, z, z_len, a, a_len, c, k, k_len, dl); break;
    default: return -1;
  }
  return 0;
}
}
