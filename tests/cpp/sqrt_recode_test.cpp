// sqrt_recode_test.cpp — the program sqrtrecode.hpp makes of the square root's exponent (p + 1) / 4: replayed over the
// integers it gives the exponent back, its first op has no squarings, every op names one of the four odd powers or
// none, and its length is what the header's count says.  Stand-alone (no HIP); built with the address and
// undefined-behaviour sanitizers by tests/test_sqrt_recode_cpu.py, which passes each fixture's p as hex.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../bgn_amd/csrc/hostbig.hpp"
#include "../../bgn_amd/csrc/sqrtrecode.hpp"

using namespace bgn;

static int check(const BigU& e, const char* what, bool report = false) {
  const std::vector<uint16_t> ops = sqrt_recode(e.w.data(), e.bits());
  if (ops.empty() || (ops[0] & 0xFF) != 0 || (ops[0] >> 8) == kSqrtNoMul) {
    printf("%s: the first op must start the accumulator\n", what);
    return 1;
  }
  BigU v;
  size_t squarings = 0, products = 0;
  for (uint16_t op : ops) {
    const uint32_t n = op & 0xFF, idx = op >> 8;
    if (idx != kSqrtNoMul && idx >= (uint32_t)kSqrtPowers) {
      printf("%s: power index %u\n", what, idx);
      return 1;
    }
    if (idx == kSqrtNoMul && n == 0) {
      printf("%s: an empty op\n", what);
      return 1;
    }
    for (uint32_t i = 0; i < n; ++i) v.shl1();
    if (idx != kSqrtNoMul) v.add_small(2 * idx + 1);
    squarings += n;
    products += idx != kSqrtNoMul;
  }
  if (BigU::cmp(v, e) != 0) {
    printf("%s: the replay is not the exponent\n", what);
    return 1;
  }
  // the squarings are the bits below the first window; windows end on set bits, so two of them span three bits at least
  const size_t bits = (size_t)e.bits();
  if (squarings >= bits || products > bits / 2 + 2) {
    printf("%s: %zu squarings, %zu products for %zu bits\n", what, squarings, products, bits);
    return 1;
  }
  if (report) printf("%s: %zu bits, %zu ops, %zu squarings, %zu products\n", what, bits, ops.size(), squarings, products - 1);
  return 0;
}

static BigU from_hex(const char* s) {
  std::string h(s);
  if (h.size() % 2) h = "0" + h;
  std::vector<uint8_t> b(h.size() / 2);
  for (size_t i = 0; i < b.size(); ++i) {
    unsigned v;
    sscanf(h.c_str() + 2 * i, "%2x", &v);
    b[i] = (uint8_t)v;
  }
  return BigU::from_be(b.data(), b.size());
}

int main(int argc, char** argv) {
  int bad = 0;
  for (int a = 1; a < argc; ++a) {              // (p + 1) / 4 of each p given
    BigU e = from_hex(argv[a]);
    e.add_small(1);
    e.shr1();
    e.shr1();
    char label[32];
    snprintf(label, sizeof label, "p[%d]", a);
    bad += check(e, label, true);
  }
  // shapes no key's exponent need have: a single bit, all ones, a run of more than 255 zeros, ones 300 bits apart
  for (uint64_t small = 1; small < 600; ++small) bad += check(BigU(small), "small");
  BigU ones;
  for (int i = 0; i < 67; ++i) {
    ones.shl1();
    ones.add_small(1);
  }
  bad += check(ones, "ones");
  BigU gap((uint64_t)5);
  for (int i = 0; i < 300; ++i) gap.shl1();
  bad += check(gap, "5 << 300");
  gap.add_small(1);
  bad += check(gap, "(5 << 300) + 1");
  puts(bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
