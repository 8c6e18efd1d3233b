// coop_api.hpp — host-visible launcher of the wave-cooperative pairing kernel (coop.hpp, kern_coop.hip).
#pragma once
#include "../kernels.hpp"

namespace bgn {
// The job's pairings (kernels.hpp PairingJob; shapes Each, Broadcast and Poly), one workgroup per pairing; operands
// canonical Montgomery SoA, results plain canonical SoA, as KernelTable::pairing.  Returns false when `nl` has no
// instantiation (then nothing was launched).  p_bits: bound on the bit length of p for the division steps.
// job.ws: workspace of coop_ws_words(nl, sw) u32 (sw >= count, the limb stride of its arrays) — the pairing then runs
// as Miller-loop kernel, batched inversion of the norms (division steps, one per lane), final-exponentiation
// kernel; job.ws == nullptr: one launch with the Fermat inversion on the waves.
// job.tab != nullptr: e(K, a[e]) over the NORMALISED line table of the key point K (fixedpair.hpp; limb stride 1) built
// for the scalar whose NAF job.consts holds; b is not read (the shape is Broadcast's).
// Not read: tab_stride, tab_normalized, curve_a3, run, window.
bool coop_pairing_launch(int nl, hipStream_t s, const void* params, int p_bits, const PairingJob& job);
size_t coop_ws_words(int nl, size_t sw);
// out[e] = a[e]^k[e] in F_p^2, one element per workgroup: a canonical Montgomery SoA (sa == 1: one base), k big-endian
// bytes (klen <= 256 each; kstride 0: one exponent), out canonical Montgomery SoA.
bool coop_gt_pow_launch(int nl, hipStream_t s, const void* params, const uint32_t* a0, const uint32_t* a1, size_t sa,
                        const uint8_t* k, size_t kstride, size_t klen, uint32_t* o0, uint32_t* o1, size_t so, size_t count);
const char* coop_pairing_kernel_name(int nl);
// Diagnostics (bgn_field_ops_family_batch): the family's field arithmetic on its own, one element per wave.  xy canonical
// Montgomery SoA (x in c0, y in c1); prod = (x*y, (x-y)*(x+y)), sqr = (x^2, y^2), lin = (x+y, x-y), plain canonical SoA.
// Returns false when `nl` has no instantiation (the limb counts of the pairing kernel); count == 0 launches nothing and
// only answers that.
bool coop_field_ops_launch(int nl, hipStream_t s, const void* params, SoA2 xy, SoA2 prod, SoA2 sqr, SoA2 lin, size_t count);
}  // namespace bgn
