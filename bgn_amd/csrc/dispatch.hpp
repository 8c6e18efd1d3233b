// dispatch.hpp — which pairing-kernel family serves a piece of work, and how a large batch is cut for it.  Host only,
// pure integer logic over the limb count, the options, the calibrated crossovers and "is there an instantiation":
// engine.cpp compares no count against a limit itself, and tests/cpp/dispatch_test.cpp pins the table without a GPU.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>

#include "options.hpp"

namespace bgn {

// lane offsets inside a limb row are 32-bit byte offsets (gmem.hpp): at most 2^28 elements per call
constexpr size_t kMaxBatch = (size_t)1 << 28;

enum class Work { Mult = 0, MakeL2 = 1, Lift = 2, Power = 3 };    // Lift / Power: Decrypt's lift, its power by the secret key
enum class Family { Lane, Coop, Quad };                           // one element per lane / per workgroup / per sixteen lanes

// Crossovers between the three pairing-kernel families, in elements per call; index = Work.  -1: the constants of the
// committed sweeps (coop_limit / quad_max below); bgn_ctx_calibrate replaces them by what two timed probes per kernel
// say on THIS device.
// (atomics: bgn_ctx_calibrate publishes them while other threads' calls read them in their dispatch)
struct Crossovers {
  std::atomic<int64_t> coop[4] = {{-1}, {-1}, {-1}, {-1}};
  std::atomic<int64_t> quad[4] = {{-1}, {-1}, {-1}, {-1}};
};

struct DispatchView {                      // what the decision reads of a context
  int nl;                                  // limbs per F_p value
  bool table_walk;                         // fixed_normalized && coop_table != 0: the key's line tables can be walked
  bool has_coop, has_quad, has_quad_mc;    // an instantiation exists for nl (cooperative; lane groups; their MultConst)
  const Options* opt;
  const Crossovers* xo;
};

namespace detail {

inline int64_t get(const DispatchView& v, Options::V Options::*f) { return (v.opt->*f).load(std::memory_order_relaxed); }

// Between the cooperative kernel's saturation and one pairing per lane filling the chip sits the lane-group kernel
// (quad/quad.hpp: sixteen lanes per pairing; 4096 pairings put one wave on every SIMD, three workgroups share a CU):
// Mult and MultPoly's coefficient pairs above coop_limit and up to quad_max pairs, from the committed sweep
// profiles/r03_mid_batch.csv (MI355X, 1024 bits: 4096 pairs 18.9 ms, 16384 54.9 ms, 49152 153.3 ms against 155.5 ms
// for ANY count up to 65536 on the lane kernel, 1024 pairs 21.2 ms against 17.8 ms cooperative; 512 bits: 4096
// pairs 5.1 ms, 40960 27.9 ms against 28.2 ms, 1024 pairs 5.2 against 5.3 ms).  A lane of the lane kernel takes a
// second pairing from 65537 pairs on: such a batch is cut into whole rounds of that kernel and a remainder that
// comes back here (rounds_head).  BGN_QUAD_MAX overrides the upper end (0 disables the kernel), BGN_QUAD_MIN
// the lower one.
// The walks over a key's line table (makeL2; Decrypt's lift) and Decrypt's power by the secret key on the lane-group
// kernel: above the cooperative crossover of the same work and up to these counts
// (profiles/r03_mid_batch_table.csv); BGN_QUAD_MAX_L2 / BGN_QUAD_MAX_DEC / BGN_QUAD_MAX_POW override, 0 disables.
inline size_t quad_max(const DispatchView& v, Work w) {
  const int mode = (int)w;
  const int64_t ov = get(v, mode == 3 ? &Options::quad_max_pow : mode == 2 ? &Options::quad_max_dec : mode == 1 ? &Options::quad_max_l2 : &Options::quad_max);
  if (ov >= 0) return (size_t)ov;
  if (!v.has_quad || (mode && !quad_max(v, Work::Mult))) return 0;    // no instantiation for this limb count; quad_max=0
  if (v.nl > 40) return kMaxBatch;      // 72 limbs: the lane kernels are the functional fallback, not the fast path
  if (v.xo->quad[mode] >= 0) return (size_t)v.xo->quad[mode];          // bgn_ctx_calibrate
  // profiles/r04_mid_batch.csv (nine-round segments, width-5 loop): 49152 pairs 128 ms, 65536 168 ms against 157 on the
  // lane kernel (512 bits: 65536 pairs 36.1 against 28.6, 49152 27.7 against 28.5); profiles/r04_calibrate.csv: 61 600 / 50 900.
  // Round 5: the lane kernel's round is 138 ms (lazy reduction), the lane groups are what they were — 49152 pairs
  // 126 ms, 65536 167 ms (profiles/r05_mid_batch.csv); profiles/r05_calibrate.csv: 55 100 ... 55 400 / 45 500
  if (mode == 0) return v.nl >= 36 ? 55000 : v.nl >= 19 ? 45500 : 32768;
  // profiles/r03_mid_batch_table.csv, whole calls at 1024 / 512 bits: Decrypt of 16384 ciphertexts 21.0 / 4.3 ms
  // against 36.6 / 6.9 on the lane kernels, of 32768 36.7 / 7.5 against 36.9 / 6.9; makeL2 of 32768 37.4 / 8.5 against
  // 53.2 / 10.6, of 65536 72.2 / 15.9 against 53.7 / 10.8
  // (round 4: profiles/r04_calibrate.csv 33 100 / 30 200 and 48 300 / 43 600; round 5, the table walks of the lane
  // kernel with two sums of two products per step: profiles/r05_calibrate.csv 31 000 / 26 900 and 45 300 / 37 700)
  if (mode == 3 || mode == 2) return v.nl >= 36 ? 31000 : v.nl >= 19 ? 26900 : 16384;
  return v.nl >= 36 ? 45300 : v.nl >= 19 ? 37700 : 16384;
}

// Small batches go to the wave-cooperative kernel (coop/coop.hpp: one pairing per workgroup of eight waves) —
// a lane of k_pairing runs a whole pairing alone, so any batch below one wave per SIMD (65536 pairings) costs
// the latency of ONE pairing there (166 ms at a 1024-bit key, 28 ms at 512 bits), while the cooperative kernel
// finishes a pairing in a few milliseconds and runs one per CU (several with more workgroups resident).
// The crossovers come from the committed sweep profiles/r02_small_batch.csv; BGN_COOP_MAX / BGN_COOP_MAX_L2
// override them (0 disables the kernel).
inline size_t coop_limit(const DispatchView& v, Work w) {
  if (!v.has_coop) return 0;      // one limb per lane of a wave: no cooperative kernel beyond 64 limbs (2048-bit keys)
  const int mode = (int)w;
  const int64_t ov = get(v, mode >= 2 ? &Options::coop_max_dec : mode == 1 ? &Options::coop_max_l2 : &Options::coop_max);
  if (ov >= 0) return (size_t)ov;
  const bool tw = v.table_walk;
  // with the lane-group kernel's table walk and power above it (profiles/r03_mid_batch_table.csv, whole calls, 1024
  // bits: Decrypt of 1024 ciphertexts 7.1 ms cooperative against 7.6, of 2048 12.3 against 7.6; makeL2 of 1024 7.9
  // against 7.1 ms; 512 bits: Decrypt 1024: 2.1 against 1.9 ms, makeL2 1024: 2.7 against 2.1) the cooperative kernel
  // keeps what is below that kernel's one-round time
  const bool quad_tw = tw && quad_max(v, Work::Mult) != 0;
  // Lift: the lane kernel walks the half-length table of the secret order (29 ms at 1024 bits, 4.5 ms at 512, whatever
  // the batch below 65536); the cooperative kernel walks the same table in two or three rounds per step (8192 lifts in
  // 13 ms at 1024 bits, 8 ms at 512) — without the table walk it runs a whole e(C, P) and wins only below ~2000 / ~800
  if (quad_tw && v.xo->coop[mode] >= 0) return (size_t)v.xo->coop[mode];        // bgn_ctx_calibrate
  if (mode == 2 || (mode == 3 && quad_tw)) {
    if (quad_tw) return v.nl >= 36 ? 1300 : v.nl >= 19 ? 740 : 512;
    return tw ? (v.nl >= 36 ? 14000 : v.nl >= 19 ? 4000 : 2048) : (v.nl >= 36 ? 2000 : v.nl >= 19 ? 800 : 512);
  }
  // Power: 1.5 rounds per bit on the waves (≈ 1 ms at 1024 bits, one element
  // per CU) against 2 products per bit on one lane (8 ms whatever the batch below 65536)
  if (mode == 3) return v.nl >= 36 ? 2048 : v.nl >= 19 ? 1024 : 512;
  // profiles/r02_small_batch.csv (MI355X): Mult at 1024 bits — 8192 pairings 114 ms cooperative against 166 ms,
  // 16384: 225 against 166; at 512 bits — 4096: 17.1 against 28.2 ms, 8192: 33.0 against 28.2.  makeL2 (both
  // kernels walk P's line table): 1024 bits — 8192: 52.5 against 54.3 ms, 16384: 103 against 54; 512 bits —
  // 4096: 8.7 against 10.6 ms, 8192: 16.7 against 10.6 (general cooperative program: 3000 / 1800).
  if (mode == 1) {
    if (quad_tw) return v.nl >= 36 ? 850 : v.nl >= 19 ? 640 : 512;
    return tw ? (v.nl >= 36 ? 8000 : v.nl >= 19 ? 4800 : 2048) : (v.nl >= 36 ? 3000 : v.nl >= 19 ? 1800 : 1024);
  }
  // Mult: with the lane-group kernel above it (profiles/r03_mid_batch.csv: 1024 pairs 17.8 ms cooperative against
  // 21.2 ms, 1536: 25.1 against 21.3 at 1024 bits; 512 bits: 1024 pairs 5.3 against 5.2 ms) the crossover is where
  // that kernel's one-round time is reached; without it, the lane kernel's (r02_small_batch.csv)
  // (round 4, 24-instruction rows, nine-round segments and the width-5 loop: profiles/r04_mid_batch.csv 1024 pairs
  // 17.0 ms cooperative against 16.0, 512 bits 5.3 against 4.5; profiles/r04_calibrate.csv puts the crossings at 950 / 815)
  if (quad_max(v, Work::Mult)) return v.xo->coop[0] >= 0 ? (size_t)v.xo->coop[0] : v.nl >= 36 ? 950 : v.nl >= 19 ? 815 : 800;
  return v.nl >= 36 ? 10000 : v.nl >= 19 ? 6000 : 4096;
}

inline size_t quad_floor(const DispatchView& v, Work w) {
  if (get(v, &Options::quad_min) >= 0) return (size_t)get(v, &Options::quad_min);
  // an explicit cooperative limit alone keeps the meaning it had before the lane-group kernel existed (the A/B switch
  // between the cooperative and the lane kernel: cooperative below it, lane kernel above; 0 = lane kernel always)
  if (w == Work::Mult ? (get(v, &Options::coop_max) >= 0 && get(v, &Options::quad_max) < 0)
                      : (get(v, w == Work::MakeL2 ? &Options::coop_max_l2 : &Options::coop_max_dec) >= 0 &&
                         get(v, &Options::quad_max_l2) < 0 && get(v, &Options::quad_max_dec) < 0 && get(v, &Options::quad_max_pow) < 0))
    return (size_t)-1;
  return coop_limit(v, w);
}

// Is `count` in the lane groups' range, availability aside?  The table walks (makeL2, the lift) need the key's
// normalised table; Mult's range is empty without an instantiation, the others' may be forced by an option.
inline bool quad_range(const DispatchView& v, Work w, size_t count) {
  if (w == Work::Mult ? !v.has_quad : (w != Work::Power && !v.table_walk)) return false;
  return count > quad_floor(v, w) && count <= quad_max(v, w);
}

}  // namespace detail

// The one decision: the kernel family that runs `count` elements of `w` in one launch.  Never a family without an
// instantiation for nl: that one is skipped, then the cooperative kernel up to its limit, else the lane kernel.
inline Family family(const DispatchView& v, Work w, size_t count) {
  if (v.has_quad && detail::quad_range(v, w, count)) return Family::Quad;
  return count <= detail::coop_limit(v, w) ? Family::Coop : Family::Lane;
}

// The lane kernel runs `pairing_run` pairings on each of at most 65536 lanes — one wave per SIMD, 512 registers — so
// its time is a step function of the count: 65537 pairs cost two pairings' latency, 2^20 + 1 pairs two rounds of
// sixteen.  A batch that does not fill whole rounds is therefore cut: the largest head that does (a multiple of
// 2^20 above 2^20, of 65536 below) goes first, the remainder follows as a call of its own and takes whichever
// kernel is fastest at ITS size (1024 bits: 70 000 Mults 310 -> 176 ms, 2^20 + 1000: 5.0 -> 2.5 s).  Below 2^20 the
// cut is made only when the remainder lands on the cooperative or the lane-group kernel (a remainder on the lane
// kernel costs the same extra round either way).  Returns the head of a batch of n.
inline size_t rounds_head(const DispatchView& v, Work w, size_t n) {
  using namespace detail;
  constexpr size_t kLanes = 65536, kFull = kLanes * 16;
  if (n <= kLanes || get(v, &Options::split_rounds) == 0) return n;
  if (quad_range(v, w, n)) return n;      // a batch the lane-group kernel takes whole — every size at 72 limbs — is not cut
  // (the power runs one element per lane, rounds of 65536 whatever the count: 1024 bits, 66 000 level-2 Decrypts 21.4 -> 13 ms)
  if (w != Work::Power && n > kFull) return n - n % kFull;
  const size_t rem = n % kLanes;
  if (!rem) return n;
  // does a smaller family take the remainder?  (the table walks and the power test the lane groups' upper end alone)
  const bool coop_rem = rem <= coop_limit(v, w), quad_rem = w == Work::Mult ? quad_range(v, w, rem) : rem <= quad_max(v, w);
  const bool small = w == Work::MakeL2 ? v.table_walk && (coop_rem || quad_rem)      // (never cut without the table walk)
                     : w == Work::Lift ? coop_rem || (v.table_walk && quad_rem) : coop_rem || quad_rem;
  return small ? n - rem : n;
}

// MultConst with per-element scalars on the lane groups (quad/quad_g1.hpp: sixteen lanes per element, level 1 a
// windowed Jacobian ladder, level 2 a windowed power in F_p^2): from ONE element on — there is no cooperative variant,
// and a lone lane of k_g1_mul / k_gt_pow needs the latency of a whole ladder (96 ms for a 1024-bit scalar at a
// 1024-bit key) — up to where one element per lane fills the chip better (profiles/r04_multconst_mid_batch.csv).
// A larger batch is cut into whole rounds of 65536 lanes for the lane kernel and a remainder that comes back here.
// Option quad_max_mc overrides (0: never).
inline size_t multconst_quad_limit(const DispatchView& v, int level, size_t klen) {
  using detail::get;
  const int64_t ov = get(v, &Options::quad_max_mc);
  if (ov >= 0) return (size_t)ov;
  if (!v.has_quad_mc) return 0;                                       // no instantiation for this limb count
  if (v.nl > 40) return kMaxBatch;                                    // 72 limbs: the lane kernels are the functional fallback
  // profiles/r04_multconst_mid_batch.csv (MI355X, 1024-bit key, ms for 49152 / 65536 elements, lane groups against one
  // element per lane): level 1, 1024-bit scalars 98 / 129 against 94 / 96; 256-bit 25.5 / 33.6 against 26.9 / 29.0;
  // 40-bit (the lane kernel's binary ladder) 5.2 / 6.7 against 6.7 / 7.0.  Level 2: 1024-bit 35.7 / 47.0 against
  // 35.5 / 35.6; 40-bit 2.1 / 2.7 against 1.5 / 1.5 (32768: 1.5 against 1.5).
  // 512-bit key, 32768 / 49152 elements: level 1, 256-bit scalars 7.6 / 10.9 against 8.5 / 9.0, 40-bit 1.6 / 2.2 against
  // 2.2 / 2.2; level 2, 256-bit 2.9 / 4.1 against 3.3 / 3.3, 40-bit 0.66 / 0.93 against 0.58 / 0.60.
  const bool short_k = klen < 16;
  // (round 4's 24-instruction rows, same file re-measured: level 1, 1024-bit scalars 49152 elements 96.0 against 93.7 ms;
  // level 2 35.0 against 35.4)
  // Round 6: on level 2 the lane kernel takes the norm-1 ladder (two products per scalar bit instead of five,
  // kernels_impl.hpp k_gt_pow) and the lane groups still square and multiply, so the lane groups win a smaller range
  // (profiles/r06_multconst_l2_crossover.csv: 1024-bit key, lane groups against lane kernel in ms,
  // 16384 / 20480 elements: 1024-bit scalars 12.6 / 15.4 against 13.6; 256-bit 3.3 / 4.0 against 3.7; 40-bit 0.72 /
  // 0.86 against 0.87 / 0.89.  512-bit key, 24576 / 32768: 256-bit 2.17 / 2.81 against 2.27; 40-bit 0.48 / 0.61
  // against 0.48 / 0.50).
  const bool ladder = level == 2 && get(v, &Options::multconst_l2_ladder) != 0;
  // Round 6, level 1 with short scalars: the lane kernel takes 2-bit windows from 3 scalar bytes on (g1_mul_launch) and
  // is 1.3x the binary ladder it replaces (profiles/r06_multconst_short.csv: 1024-bit key, lane groups against lane
  // kernel in ms at 49152 / 57344 elements: 40-bit 4.98 / 5.74 against 5.18; 64-bit 7.19 / 8.31 against 7.75; 120-bit
  // 12.3 / 14.2 against 13.7; 8-bit (binary ladder) at 32768: 1.57 against 1.54.  512-bit key at 40960: 40-bit 1.82
  // against 1.81, 120-bit 4.40 against 4.75; 8-bit at 16384 / 32768: 0.42 / 0.65 against 0.53).
  const bool tiny_k = klen < 3;
  const bool short_win = short_k && !tiny_k && get(v, &Options::g1_mul_window_short) != 0;
  if (v.nl >= 36)
    return level == 1 ? (tiny_k ? 32768 : short_win ? 51000 : short_k ? 65536 : 47000)
                      : ladder ? (short_k ? 21000 : 17500) : (short_k ? 32768 : 49000);
  if (v.nl >= 19)
    return level == 1 ? (tiny_k ? 24000 : short_win ? 41000 : short_k ? 48000 : 38000)
                      : ladder ? (short_k ? 24000 : 26000) : (short_k ? 28000 : 37000);
  return level == 1 ? 32768 : 24576;
}

// Segmented sums (sumops.hpp): nseg segments of seg_len elements are folded by reduction passes, pass k leaving
// split[k] partials per segment (lane (s, t) of a pass accumulates the elements t, t + split, ... of segment s); the
// last pass has split 1.  Two wishes pull at the choice: a chip wants `chip_lanes` lanes busy (level 1: 65536, one wave
// on every SIMD; level 2: twice that), and a lane wants a run of at least `run_min` elements, over which its one
// conversion per pass (level 1: the inversion that makes the Jacobian accumulator affine, about three additions'
// worth) is spread.  While the array is large enough for both, a pass takes just the lanes that fill the chip and the
// runs are as long as that leaves them; below, runs of run_min and fewer lanes — those passes are bound by the latency
// of a run, and short runs in more passes beat long ones (1 x 2^20 at a 1024-bit key, run_min 2 / 4 / 8 / 16: level 1
// 10.7 / 8.2 / 8.5 / 10.1 ms, level 2 0.92 / 1.01 / 1.26 / 1.83 ms, profiles/r10_sum_rates.csv; engine.cpp passes 4
// and 2).
// forced >= 1: the first pass's split, clamped to seg_len (a split equal to the length is a pass that only copies);
// the passes behind it are planned.
struct SumPlan {
  int passes = 0;
  uint32_t split[32] = {};
};

inline SumPlan plan_sum(size_t nseg, size_t seg_len, size_t chip_lanes, int64_t forced, int64_t run_min) {
  SumPlan p;
  if (!nseg || !seg_len) return p;
  const size_t rmin = run_min < 2 ? 2 : (size_t)run_min;
  if (!chip_lanes) chip_lanes = 1;
  size_t len = seg_len;
  for (;;) {
    size_t split;
    if (p.passes == 0 && forced >= 1) {
      split = (size_t)forced < len ? (size_t)forced : len;
    } else {
      const size_t by_run = len / rmin;                                  // lanes per segment with runs of rmin
      const size_t by_chip = (chip_lanes + nseg - 1) / nseg;              // lanes per segment that fill the chip
      split = by_run < by_chip ? by_run : by_chip;
      size_t pw = 1;
      while (pw * 2 <= split) pw *= 2;                                   // whole workgroups, or whole segments per workgroup
      split = pw;
    }
    p.split[p.passes++] = (uint32_t)split;
    if (split == 1) break;
    len = split;
    if (p.passes == 31) {                                                // (never: a planned pass at least halves the length)
      p.split[p.passes++] = 1;
      break;
    }
  }
  return p;
}

}  // namespace bgn
