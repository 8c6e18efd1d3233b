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

// Linear maps (linops.hpp): out[v][r] = sum_j w[r][j] * ct[v][j] over nvec vectors of d ciphertexts and nrows rows of
// weights below 2^w_bits.  Two choices, neither of which any byte depends on:
//   omega   the window width, 1 .. 8.  A table of the multiples 1 .. H = 2^(omega-1) of every ciphertext costs
//           ncols * (H-1) table steps (ncols = nvec*d, one lane per ciphertext) and has to fit `budget_bytes` at
//           `entry_bytes` per entry, and 2^28 entries (gmem.hpp); the walk then costs every output d * nwin additions
//           and (nwin-1) * omega doublings, nwin = ceil((w_bits+1) / omega).  omega = 1 needs no table.
//   nchunk  the chunks the columns of one output are cut into, each a lane of its own whose partial the passes of
//           plan_sum fold afterwards: as many as fill `chip_lanes` lanes, while a chunk keeps at least kLinMinRun columns
//           to spread its doublings and its one inversion over.
// Costs are in rounds of the chip: work that fits the chip's lanes once takes as long as one lane's.  The unit is one
// F_p product: a mixed addition 13, a doubling 9, a table step 13 + 6 (the entry's share of the shared inversion), a
// lane's conversion about 40; level 2: a product in F_p^2 3, a squaring 2, no conversion.
// forced_window in 1 .. 8 and forced_split >= 1 override (the window narrowed until its table fits; the split clamped
// to d and to 2^28 partials).
constexpr size_t kLinMinRun = 8;
// (this header includes nothing of the kernels': the widest window and the window count are restated from linrecode.hpp,
// and tests/cpp/lin_recode_test.cpp holds the two against each other)
constexpr int kLinPlanMaxWindow = 8;
inline int lin_plan_windows(int w_bits, int omega) { return (w_bits + omega) / omega; }      // ceil((w_bits + 1) / omega)
struct LinCost {
  double c_table, c_add, c_dbl, c_fin;
};
inline LinCost lin_cost(int level) { return level == 1 ? LinCost{19, 13, 9, 40} : LinCost{3, 3, 2, 2}; }

struct LinPlan {
  int omega = 0, nwin = 0;
  size_t nchunk = 0;
  size_t entries = 0;           // table entries (0 at omega = 1)
};

inline size_t lin_table_entries(size_t ncols, int omega) { return omega > 1 ? ncols << (omega - 1) : 0; }

inline LinPlan plan_lincomb(size_t nvec, size_t nrows, size_t d, int w_bits, size_t budget_bytes, size_t entry_bytes,
                            int level, size_t chip_lanes, int64_t forced_window, int64_t forced_split) {
  LinPlan p;
  if (!nvec || !nrows || !d || w_bits < 1 || w_bits > 31) return p;
  if (!chip_lanes) chip_lanes = 1;
  const size_t ncols = nvec * d, nout = nvec * nrows;
  // chunks
  size_t nchunk = 1;
  if (forced_split >= 1) {
    nchunk = (size_t)forced_split;
  } else if (nout < chip_lanes) {
    const size_t by_chip = (chip_lanes + nout - 1) / nout, by_run = d / kLinMinRun;
    nchunk = by_run < by_chip ? by_run : by_chip;
  }
  if (nchunk > d) nchunk = d;
  if (nchunk > kMaxBatch / nout) nchunk = kMaxBatch / nout;
  if (nchunk < 1) nchunk = 1;
  p.nchunk = nchunk;
  // window
  const LinCost k = lin_cost(level);
  const auto fits = [&](int omega) {
    const size_t e = lin_table_entries(ncols, omega);
    return omega == 1 || (e <= kMaxBatch && entry_bytes <= budget_bytes && e <= budget_bytes / entry_bytes);
  };
  const auto rounds = [&](size_t lanes) { return (double)((lanes + chip_lanes - 1) / chip_lanes); };
  int best = 1;
  if (forced_window >= 1) {
    best = forced_window > kLinPlanMaxWindow ? kLinPlanMaxWindow : (int)forced_window;
    while (!fits(best)) --best;
  } else {
    double best_cost = 0;
    for (int omega = 1; omega <= kLinPlanMaxWindow; ++omega) {
      if (!fits(omega)) break;
      const int nwin = lin_plan_windows(w_bits, omega);
      const double H = (double)((size_t)1 << (omega - 1));
      const double run = (double)((d + nchunk - 1) / nchunk);
      const double table = omega > 1 ? rounds(ncols) * (H - 1) * k.c_table : 0;
      const double walk = rounds(nout * nchunk) * (run * nwin * k.c_add + (double)(nwin - 1) * omega * k.c_dbl + k.c_fin);
      const double cost = table + walk;
      if (omega == 1 || cost < best_cost) {
        best = omega;
        best_cost = cost;
      }
    }
  }
  p.omega = best;
  p.nwin = lin_plan_windows(w_bits, best);
  p.entries = lin_table_entries(ncols, best);
  return p;
}

// The bucket method for the same map (bucketops.hpp): no table; per (row, window) the columns are sorted into H buckets
// by digit, the buckets summed in runs of R by ceil(log_R d) reduce passes, and the bucket sums folded.  Priced in the
// units of plan_lincomb, step by step as built:
//   sort     three launches of one thread per (row, column), nwin atomics each: bkt_sort_cost products per window and
//            round — set from the sort's share of the 1 x 1 x 2^20 rows of profiles/r14_bucket_lincomb_rates.csv;
//   reduce   pass p launches nvec * nruns[p] lanes (the bound the host knows: nruns[0] = nrows * nwin * (ceil(d/R) + H),
//            nruns[p] = ceil(nruns[p-1] / R) + nb), a lane costs R additions and its conversion;
//   fold     stage 1: min(g, H) additions and a conversion, stage 2 (H > g): H/g additions and a conversion, stage 3:
//            nwin * omega doublings and additions and the final conversion — the dependent depth that is built.
// Buckets are per row and nothing is shared between rows, so every term grows with nrows: the estimate never falls as
// nrows grows at fixed d, while the table path's table is paid once.  The window and R are the cheapest admissible
// pair: the lists' slots must fit 32-bit cursors, the partials 2^28 elements, the workspace `budget_bytes` (at
// `elem_bytes` per partial).  `table_cost` prices the plan of plan_lincomb the same way, with the fold of its chunks by
// plan_sum, and the buckets are taken where they are cheaper by kBktMargin — never below kBktMinCols columns: the profile
// has a gain at 2^20 columns under one row and none at 2^18 under four, 2^14 under 64 or 1024 under 1024, and nothing
// between was measured — always or never with lin_buckets = 1 / 0.  A forced window is clamped to 1 .. 8, a forced R to 2 .. kBktMaxRun; a forced pair that is not
// admissible leaves use = false: the caller falls back to the table path.
constexpr size_t kBktMinCols = (size_t)1 << 20;
constexpr double kBktMargin = 0.95;        // the estimates are good to about 5 %: a tie stays with the tables
constexpr int64_t kBktMaxRun = 256;
constexpr int kBktFoldGroup = 16;
constexpr int kBktMaxPasses = 28;          // R >= 2, d <= 2^28
// The sort, per window and round of 65536 (row, column) threads, in products: the milliseconds per window the sort of
// 2^20 columns of one row measured under every window (profiles/r14_bucket_lincomb_rates.csv, rows "lin_bucket_window
// 4 .. 8" and the 8-bit rows; 16 rounds; narrower windows, where still more columns meet in one cursor, are priced as 4),
// over what a product of the table path measures there (11.3 us on level 1, 17 us on level 2).
inline double bkt_sort_cost(int level, int omega) {
  static const double ms[kLinPlanMaxWindow + 1] = {0, 2.2, 2.2, 2.2, 2.2, 2.2, 1.25, 1.85, 2.1};
  return ms[omega] / 16 / (level == 1 ? 0.0113 : 0.017);
}
// A lane-round of the reduce passes and the fold against one of the walk, per product counted: every step is one
// addition of an element that is read once, with no digit plane and no table gather (1 x 1 x 2^20 at 16 bits: 19.8 ms for
// 2478 products on level 1, 5.6 ms for 462 on level 2, against 11.1 and 18 us per product of the table path).
constexpr double kBktLaneRate = 0.72;

struct BktPlan {
  bool use = false;
  int omega = 0, nwin = 0, npass = 0;
  uint32_t R = 0;
  int nc = 0;                              // groups of kBktFoldGroup buckets per window
  size_t nb = 0;                           // buckets: nrows * nwin * H
  size_t nruns[kBktMaxPasses] = {};        // runs per vector of pass p (bound)
  size_t cap[2] = {};                      // elements per vector of the two arrays of partials: passes in turns, then the fold
  size_t bytes = 0;                        // the path's workspace beyond the decoded vectors and the tail's arrays
  double cost = 0, table_cost = 0;
};

inline int bkt_passes(size_t d, size_t R) {
  int n = 1;
  for (size_t len = (d + R - 1) / R; len > 1; len = (len + R - 1) / R) ++n;
  return n;
}

// The shape of the path at (omega, R); false where the kernels cannot run it.
inline bool bkt_shape(BktPlan& p, size_t nvec, size_t nrows, size_t d, int w_bits, int omega, size_t R, size_t elem_bytes) {
  const size_t H = (size_t)1 << (omega - 1);
  p.omega = omega;
  p.nwin = lin_plan_windows(w_bits, omega);
  p.R = (uint32_t)R;
  p.nc = (int)((H + kBktFoldGroup - 1) / kBktFoldGroup);
  p.nb = nrows * (size_t)p.nwin * H;
  p.npass = bkt_passes(d, R);
  p.nruns[0] = nrows * (size_t)p.nwin * ((d + R - 1) / R + H);
  for (int k = 1; k < p.npass; ++k) p.nruns[k] = (p.nruns[k - 1] + R - 1) / R + p.nb;
  if (p.nruns[0] > 0xffffffffu / R || p.nruns[0] > kMaxBatch / nvec) return false;
  p.cap[0] = p.cap[1] = p.nb;                                                // (a stage of the fold writes at most nb per vector)
  for (int k = 0; k < p.npass; ++k)
    if (p.nruns[k] > p.cap[k & 1]) p.cap[k & 1] = p.nruns[k];
  if (p.cap[0] > kMaxBatch / nvec || p.cap[1] > kMaxBatch / nvec) return false;
  p.bytes = p.nruns[0] * R * 4 + (2 * (size_t)p.npass + 2) * p.nb * 4 + (nvec * (p.cap[0] + p.cap[1]) + 128) * elem_bytes + 4096;
  return true;
}

inline double bkt_cost(const BktPlan& p, size_t nvec, size_t nrows, size_t d, int level, size_t chip_lanes) {
  const LinCost k = lin_cost(level);
  const auto rounds = [&](size_t lanes) { return (double)((lanes + chip_lanes - 1) / chip_lanes); };
  const size_t H = (size_t)1 << (p.omega - 1), nout = nvec * nrows, nq = nout * (size_t)p.nwin * (size_t)p.omega;
  double c = 0;
  // (of the nruns[i] lanes launched, at most nruns[i] - nb runs are full; the others end early or exit at once)
  for (int i = 0; i < p.npass; ++i) c += rounds(nvec * (p.nruns[i] - p.nb)) * (p.R * k.c_add + k.c_fin);
  c += rounds(nq * (size_t)p.nc) * ((double)(H < (size_t)kBktFoldGroup ? H : (size_t)kBktFoldGroup) * k.c_add + k.c_fin);
  if (p.nc > 1) c += rounds(nq) * (p.nc * k.c_add + k.c_fin);
  c += rounds(nout) * ((double)p.nwin * p.omega * (k.c_dbl + k.c_add) + k.c_fin);
  return c * kBktLaneRate + rounds(nrows * d) * p.nwin * bkt_sort_cost(level, p.omega);
}

// What plan_lincomb's plan costs, the fold of its chunks included.
inline double lin_table_cost(const LinPlan& t, size_t nvec, size_t nrows, size_t d, int level, size_t chip_lanes) {
  const LinCost k = lin_cost(level);
  const auto rounds = [&](size_t lanes) { return (double)((lanes + chip_lanes - 1) / chip_lanes); };
  const size_t nout = nvec * nrows;
  const double H = (double)((size_t)1 << (t.omega - 1)), run = (double)((d + t.nchunk - 1) / t.nchunk);
  double c = (t.omega > 1 ? rounds(nvec * d) * (H - 1) * k.c_table : 0) +
             rounds(nout * t.nchunk) * (run * t.nwin * k.c_add + (double)(t.nwin - 1) * t.omega * k.c_dbl + k.c_fin);
  if (t.nchunk > 1) {
    const SumPlan f = plan_sum(nout, t.nchunk, level == 1 ? chip_lanes : 2 * chip_lanes, -1, level == 1 ? 4 : 2);
    size_t len = t.nchunk;
    for (int i = 0; i < f.passes; ++i) {
      c += rounds(nout * f.split[i]) * ((double)((len + f.split[i] - 1) / f.split[i]) * k.c_add + k.c_fin);
      len = f.split[i];
    }
  }
  return c;
}

inline BktPlan plan_lincomb_buckets(size_t nvec, size_t nrows, size_t d, int w_bits, size_t budget_bytes, size_t entry_bytes,
                                    size_t elem_bytes, int level, size_t chip_lanes, int64_t forced_window, int64_t forced_split,
                                    int64_t buckets, int64_t bucket_window, int64_t bucket_run) {
  BktPlan best;
  if (!nvec || !nrows || !d || w_bits < 1 || w_bits > 31) return best;
  if (!chip_lanes) chip_lanes = 1;
  const LinPlan t = plan_lincomb(nvec, nrows, d, w_bits, budget_bytes, entry_bytes, level, chip_lanes, forced_window, forced_split);
  const double table_cost = lin_table_cost(t, nvec, nrows, d, level, chip_lanes);
  const int w0 = bucket_window >= 1 ? (int)(bucket_window > kLinPlanMaxWindow ? kLinPlanMaxWindow : bucket_window) : 1;
  const int w1 = bucket_window >= 1 ? w0 : kLinPlanMaxWindow;
  const size_t r0 = bucket_run >= 1 ? (size_t)(bucket_run < 2 ? 2 : bucket_run > kBktMaxRun ? kBktMaxRun : bucket_run) : 2;
  const size_t r1 = bucket_run >= 1 ? r0 : 64;
  bool found = false;
  for (int omega = w0; omega <= w1; ++omega)
    for (size_t R = r0; R <= r1; R *= 2) {
      BktPlan p;
      if (!bkt_shape(p, nvec, nrows, d, w_bits, omega, R, elem_bytes) || p.bytes > budget_bytes) continue;
      p.cost = bkt_cost(p, nvec, nrows, d, level, chip_lanes);
      if (!found || p.cost < best.cost) best = p;
      found = true;
    }
  best.table_cost = table_cost;
  best.use = found && buckets != 0 && (buckets > 0 || (d >= kBktMinCols && best.cost < kBktMargin * table_cost));
  return best;
}

// Column groups for the same map under narrow weights (groupops.hpp): g consecutive ciphertexts share a table of their
// M = (3^g - 1) / 2 signed combinations, and an output costs one addition per group and bit plane.  Priced in the units of
// plan_lincomb:
//   table    one lane per group (ngr = nvec * ceil(d / g) lanes), M entries each: on level 1 an affine addition of a
//            shared-inversion run (grp_step: 7 products) and g inversions of c_fin; on level 2 one product in F_p^2;
//   walk     nout * nchunk lanes; a lane adds ceil(ngroups / nchunk) * w_bits entries, doubles w_bits - 1 times, converts;
//   fold     of the chunks by plan_sum, as lin_table_cost prices it.
// The table is a dependent chain of M steps on few lanes, so the path pays only where the walk it shortens is longer
// than that chain: many rows under a long vector.  `groups`: 0 never; 2 .. 6 that group size (other positive values
// clamped), always; -1 the cheapest size, taken where nrows >= kGrpMinRows, d >= kGrpMinCols and the estimate is below
// kGrpMargin of lin_table_cost.  Either way g is narrowed until nvec * ngroups * M entries fit `budget_bytes` at `entry_bytes` each
// and 2^28 elements; if g = 2 does not fit, or w_bits > kGrpPlanMaxBits, use = false: the table path.  `table` is
// plan_lincomb's plan under the same arguments, whatever is decided.
// forced_split >= 1: the chunk count, clamped to the number of groups (chunks are whole groups).
constexpr int kGrpPlanMaxBits = 4;         // (restated from grprecode.hpp, as the window constants above)
constexpr int kGrpPlanMinGroup = 2, kGrpPlanMaxGroup = 6;
// profiles/r15_group_lincomb_rates.csv (MI355X, 1024-bit key): 1 x 4096 x 4096 and 1 x 16384 x 1024 gain at one and two
// bits on both levels (level 1, one bit: 12.6 against 27.5 ms and 11.6 against 26.2 ms, at the planned g = 4);
// 1 x 1024 x 1024, 64 x 16 x 256 and 1 x 16 x 1024 lose at every group size tried (the table's chain alone is 3.4 ms at
// g = 4 and 9 ms at g = 5 on level 1, where the whole table path takes 5 ms), and nothing between was measured: the floors
// are the smallest row and column counts with a measured gain.  The estimates at the gaining shapes are 0.4 .. 0.7 of
// the tables', at the losing ones 0.85 and more.
constexpr size_t kGrpMinRows = 4096, kGrpMinCols = 1024;
constexpr double kGrpMargin = 0.8;
inline size_t grp_plan_entries(int g) {
  size_t p = 1;
  for (int i = 0; i < g; ++i) p *= 3;
  return (p - 1) / 2;
}

struct GrpPlan {
  bool use = false;
  int g = 0;
  size_t M = 0, ngroups = 0, nchunk = 0;
  size_t entries = 0;                      // nvec * ngroups * M
  double cost = 0, table_cost = 0;
  LinPlan table;
};

inline bool grp_shape(GrpPlan& p, size_t nvec, size_t nrows, size_t d, int w_bits, int g, size_t budget_bytes, size_t entry_bytes,
                      size_t chip_lanes, int64_t forced_split) {
  p.g = g;
  p.M = grp_plan_entries(g);
  p.ngroups = (d + (size_t)g - 1) / (size_t)g;
  const size_t ngr = nvec * p.ngroups, nout = nvec * nrows;
  if (ngr > kMaxBatch / p.M || entry_bytes > budget_bytes || ngr * p.M > budget_bytes / entry_bytes) return false;
  p.entries = ngr * p.M;
  size_t nchunk = 1;
  if (forced_split >= 1) {
    nchunk = (size_t)forced_split;
  } else if (nout < chip_lanes) {
    const size_t by_chip = (chip_lanes + nout - 1) / nout, by_run = p.ngroups * (size_t)w_bits / kLinMinRun;
    nchunk = by_run < by_chip ? by_run : by_chip;
  }
  if (nchunk > p.ngroups) nchunk = p.ngroups;
  if (nchunk > kMaxBatch / nout) nchunk = kMaxBatch / nout;
  if (nchunk < 1) nchunk = 1;
  p.nchunk = nchunk;
  return true;
}

inline double grp_cost(const GrpPlan& p, size_t nvec, size_t nrows, int w_bits, int level, size_t chip_lanes) {
  const LinCost k = lin_cost(level);
  const auto rounds = [&](size_t lanes) { return (double)((lanes + chip_lanes - 1) / chip_lanes); };
  const size_t nout = nvec * nrows;
  const double grp_step = level == 1 ? 7 : 3, run = (double)((p.ngroups + p.nchunk - 1) / p.nchunk);
  double c = rounds(nvec * p.ngroups) * ((double)p.M * grp_step + (level == 1 ? p.g * k.c_fin : 0)) +
             rounds(nout * p.nchunk) * (run * w_bits * k.c_add + (double)(w_bits - 1) * k.c_dbl + k.c_fin);
  if (p.nchunk > 1) {
    const SumPlan f = plan_sum(nout, p.nchunk, level == 1 ? chip_lanes : 2 * chip_lanes, -1, level == 1 ? 4 : 2);
    size_t len = p.nchunk;
    for (int i = 0; i < f.passes; ++i) {
      c += rounds(nout * f.split[i]) * ((double)((len + f.split[i] - 1) / f.split[i]) * k.c_add + k.c_fin);
      len = f.split[i];
    }
  }
  return c;
}

inline GrpPlan plan_lincomb_groups(size_t nvec, size_t nrows, size_t d, int w_bits, size_t budget_bytes, size_t entry_bytes,
                                   int level, size_t chip_lanes, int64_t forced_window, int64_t forced_split, int64_t groups) {
  GrpPlan best;
  if (!nvec || !nrows || !d || w_bits < 1 || w_bits > 31) return best;
  if (!chip_lanes) chip_lanes = 1;
  best.table = plan_lincomb(nvec, nrows, d, w_bits, budget_bytes, entry_bytes, level, chip_lanes, forced_window, forced_split);
  best.table_cost = lin_table_cost(best.table, nvec, nrows, d, level, chip_lanes);
  if (groups == 0 || w_bits > kGrpPlanMaxBits) return best;
  const bool forced = groups > 0;
  const int g1 = !forced ? kGrpPlanMaxGroup
                         : (int)(groups < kGrpPlanMinGroup ? kGrpPlanMinGroup : groups > kGrpPlanMaxGroup ? kGrpPlanMaxGroup : groups);
  bool found = false;
  for (int g = g1; g >= kGrpPlanMinGroup; --g) {
    GrpPlan p;
    if (!grp_shape(p, nvec, nrows, d, w_bits, g, budget_bytes, entry_bytes, chip_lanes, forced_split)) continue;
    p.cost = grp_cost(p, nvec, nrows, w_bits, level, chip_lanes);
    if (!found || p.cost < best.cost) {
      p.table = best.table;
      p.table_cost = best.table_cost;
      best = p;
    }
    found = true;
    if (forced) break;                     // the widest size that fits, at most the one asked for
  }
  best.use = found && (forced || (nrows >= kGrpMinRows && d >= kGrpMinCols && best.cost < kGrpMargin * best.table_cost));
  return best;
}

// Which of the three paths of bgn_lincomb_batch runs: a forced bucket path wins over everything, a forced group size
// over planned buckets, planned buckets (long vectors under few rows) over planned groups (many rows).
enum class LinPath { Tables, Buckets, Groups };
inline LinPath lin_path(const BktPlan& b, const GrpPlan& g, int64_t buckets, int64_t groups) {
  if (buckets > 0 && b.use) return LinPath::Buckets;
  if (groups > 0 && g.use) return LinPath::Groups;
  if (b.use) return LinPath::Buckets;
  return g.use ? LinPath::Groups : LinPath::Tables;
}

// Sparse linear maps (sparseops.hpp): out[v][r] = sum_{e in row r} w[e] * ct[v][col[e]], nnz entries in rows of at most
// row_max.  The planner counts nonzeros, not nrows * d, and never sees the index arrays: a lane's run is taken at its
// bound rm = min(row_max, nnz) (a wave costs its longest row anyway).  The constants are those of plan_lincomb.
//   nchunk  the chunks a row's entries are cut into evenly, one lane each, folded by the passes of plan_sum: as many as
//           fill `chip_lanes` lanes while a chunk keeps kLinMinRun entries; and at least ceil(rm / kSpMaxRun), so that no
//           wave carries a run of more than kSpMaxRun additions per window while the rest of the chip idles (at that
//           length the lane's own doublings and conversion are below a hundredth of its run).  1 <= nchunk <= rm.
//   omega   a lane costs nwin * (9 omega + 13 ceil(rm / nchunk)) + 40 (level 2: 2, 3, 2), the tables nvec*d * (H-1)
//           steps within `budget_bytes` and 2^28 entries.  A table pays only when several rows read a column: with
//           nnz <= d no column is shared on average and the planned window is 1 (the decoded vector is the table).
// Known limit: rows are cut evenly and a wave costs its longest row, so one giant row among short ones wastes lanes —
// every row gets nchunk lanes, most of them empty.  Splitting by entries across row boundaries is not done.
// forced_window in 1 .. 8 and forced_split >= 1 override (the window narrowed until its table fits; the split clamped
// to rm and to 2^28 partials).
constexpr size_t kSpMaxRun = 1024;

inline LinPlan plan_sparse_lincomb(size_t nvec, size_t nrows, size_t d, size_t nnz, size_t row_max, int w_bits,
                                   size_t budget_bytes, size_t entry_bytes, int level, size_t chip_lanes,
                                   int64_t forced_window, int64_t forced_split) {
  LinPlan p;
  if (!nvec || !nrows || !d || w_bits < 1 || w_bits > 31) return p;
  if (!chip_lanes) chip_lanes = 1;
  const size_t ncols = nvec * d, nout = nvec * nrows;
  const size_t rm = row_max < nnz ? row_max : nnz;
  // chunks
  size_t nchunk = 1;
  if (forced_split >= 1) {
    nchunk = (size_t)forced_split;
  } else {
    if (nout < chip_lanes) {
      const size_t by_chip = (chip_lanes + nout - 1) / nout, by_run = rm / kLinMinRun;
      nchunk = by_run < by_chip ? by_run : by_chip;
    }
    const size_t by_wave = (rm + kSpMaxRun - 1) / kSpMaxRun;
    if (nchunk < by_wave) nchunk = by_wave;
  }
  if (nchunk > rm) nchunk = rm;
  if (nchunk > kMaxBatch / nout) nchunk = kMaxBatch / nout;
  if (nchunk < 1) nchunk = 1;
  p.nchunk = nchunk;
  // window
  const LinCost k = lin_cost(level);
  const auto fits = [&](int omega) {
    const size_t e = lin_table_entries(ncols, omega);
    return omega == 1 || (e <= kMaxBatch && entry_bytes <= budget_bytes && e <= budget_bytes / entry_bytes);
  };
  const auto rounds = [&](size_t lanes) { return (double)((lanes + chip_lanes - 1) / chip_lanes); };
  int best = 1;
  if (forced_window >= 1) {
    best = forced_window > kLinPlanMaxWindow ? kLinPlanMaxWindow : (int)forced_window;
    while (!fits(best)) --best;
  } else if (nnz > d) {
    double best_cost = 0;
    const double run = (double)((rm + nchunk - 1) / nchunk);
    for (int omega = 1; omega <= kLinPlanMaxWindow; ++omega) {
      if (!fits(omega)) break;
      const int nwin = lin_plan_windows(w_bits, omega);
      const double H = (double)((size_t)1 << (omega - 1));
      const double table = omega > 1 ? rounds(ncols) * (H - 1) * k.c_table : 0;
      const double walk = rounds(nout * nchunk) * (nwin * (omega * k.c_dbl + run * k.c_add) + k.c_fin);
      const double cost = table + walk;
      if (omega == 1 || cost < best_cost) {
        best = omega;
        best_cost = cost;
      }
    }
  }
  p.omega = best;
  p.nwin = lin_plan_windows(w_bits, best);
  p.entries = lin_table_entries(ncols, best);
  return p;
}

// Prefix sums (scanops.hpp): reduce, then scan.  Level k of the recursion scans nseg segments of len[k] elements in
// chunks of c[k] (one lane per chunk; a segment's last chunk may be shorter): a launch leaves the chunk totals, level
// k + 1 scans those — len[k+1] = ceil(len[k] / c[k]) per segment — and a second launch of level k applies them.  The
// last level has one chunk per segment and needs no totals.  The choice of c:
//   * a pass wants `chip_lanes` lanes busy: while the array is larger than that, c = ceil(len / ceil(chip_lanes / nseg));
//   * a lane's run carries its one inversion (level 1) and the launches of the level below: c >= run_min, and c >= 2
//     always, so that every level at least halves the length and the recursion ends;
//   * the forward sweep of level 1 keeps four field elements per element of the lanes of one launch in the workspace,
//     and the smallest launch is one workgroup: c <= max_chunk (0: no bound), which wins over run_min and the chip.
// forced >= 1: c of the FIRST level, clamped like a planned one to [2, len] and to max_chunk; the levels below are
// planned.  No byte of the result depends on any of this.
struct ScanPlan {
  int levels = 0;
  uint32_t len[32] = {};
  uint32_t c[32] = {};
  uint32_t nch[32] = {};       // chunks per segment: ceil(len / c); 1 on the last level
};

inline ScanPlan plan_scan(size_t nseg, size_t seg_len, size_t chip_lanes, int64_t run_min, int64_t forced, size_t max_chunk) {
  ScanPlan p;
  if (!nseg || !seg_len) return p;
  const size_t rmin = run_min < 2 ? 2 : (size_t)run_min;
  if (!chip_lanes) chip_lanes = 1;
  if (max_chunk == 1) max_chunk = 2;                                     // (the recursion has to shrink)
  size_t len = seg_len;
  for (;;) {
    size_t c;
    if (p.levels == 0 && forced >= 1) {
      c = (size_t)forced;
    } else {
      const size_t by_chip = (chip_lanes + nseg - 1) / nseg;              // chunks per segment that fill the chip
      c = (len + by_chip - 1) / by_chip;
      if (c < rmin) c = rmin;
    }
    if (max_chunk && c > max_chunk) c = max_chunk;
    if (c < 2) c = 2;
    if (c > len) c = len;
    const size_t nch = (len + c - 1) / c;
    p.len[p.levels] = (uint32_t)len;
    p.c[p.levels] = (uint32_t)c;
    p.nch[p.levels] = (uint32_t)nch;
    ++p.levels;
    if (nch == 1) break;
    len = nch;                                                           // (at most ceil(len / 2): 28 levels for 2^28)
  }
  return p;
}

}  // namespace bgn
