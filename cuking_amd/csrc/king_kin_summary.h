// Kinship summary (cuking_compute_kin_summary): the definitions the kernel epilogue
// (king_mfma.hip summarise_kin), the C ABI helpers (king_host.cc) and the host tests
// share, so that they cannot drift apart.  Plain C++ without a HIP header; usable from
// host and device.
//
// Histogram.  cuking_kin_bins {lo, hi, num_bins}, lo < hi, both finite, 1 <= num_bins <=
// CUKING_KIN_BINS_MAX.  A histogram has num_bins + 3 slots of uint64: slot 0 UNDER, slots
// 1 .. num_bins the bins, slot num_bins + 1 OVER, slot num_bins + 2 NAN.  The slot of a
// float32 kinship is DEFINED by kin_bin_slot() below: float32 operations, one rounding
// each, nothing fused, with scale = (float)num_bins / (hi - lo) computed once per call on
// the host (kin_bin_scale()).  The nominal edges lo + b (hi - lo) / num_bins are
// approximate -- a kinship within a rounding of an edge may land on either side of it; the
// expression is the contract.  -inf lands in UNDER, +inf and everything from hi on in
// OVER: with hi = 0.5 exact duplicates (kin 0.5) are counted in OVER.
//
// Nearest relative.  One uint64 key per sample, merged by unsigned maximum: the high word
// is the order-preserving map of the kinship's bits (bits ^ 0x80000000 for a non-negative
// float, ~bits for a negative one), the low word ~partner (the partner's GLOBAL sample
// index), so that the larger kinship wins and, among equal kinships, the lower partner.
// A NaN kinship never makes a key; key 0 = "no partner with a defined kinship" (no real
// key is 0: -inf maps to the high word 0x007FFFFF).
//
// Out of scope: the C++ `cuking` binary; merging across ranks (the tiles form and the merge
// rules -- histograms by sum, keys by maximum -- make it possible later); the VALU and
// stream kernels and bitsets from 2^24 sites on; IBS0/1/2 summaries.
//
// Relative counts (cuking_compute_relative_counts).  1 .. CUKING_REL_THRESHOLDS_MAX finite
// float32 thresholds, strictly ascending.  The BAND of a kinship is the largest t with
// kin > thresholds[t] -- the strict float32 comparison a record's `kin > kin_threshold`
// makes --, kRelNoBand (0xFFFFFFFF) when there is none: NaN and -inf never get a band.
// rel_band() below is THE definition: the refine kernel (king_filter.hip), the matrix-core
// kernels' counting epilogue (king_mfma.hip count_relatives), cuking_rel_band and the tests
// share it.
#ifndef CUKING_AMD_KING_KIN_SUMMARY_H_
#define CUKING_AMD_KING_KIN_SUMMARY_H_

#include <stdint.h>

#include "cuking_amd.h"

#if defined(__HIPCC__)
#define CUKING_SUMMARY_HD __host__ __device__
#else
#define CUKING_SUMMARY_HD
#endif

namespace cuking {

CUKING_SUMMARY_HD inline uint32_t kin_float_bits(float x) {
  uint32_t b;
  __builtin_memcpy(&b, &x, sizeof(b));
  return b;
}
CUKING_SUMMARY_HD inline float kin_bits_float(uint32_t b) {
  float x;
  __builtin_memcpy(&x, &b, sizeof(x));
  return x;
}
CUKING_SUMMARY_HD inline bool kin_is_finite(float x) {
  return (kin_float_bits(x) & 0x7F800000u) != 0x7F800000u;
}

// ---- bins ------------------------------------------------------------------------------
CUKING_SUMMARY_HD inline uint32_t kin_hist_slots(uint32_t num_bins) { return num_bins + 3; }
CUKING_SUMMARY_HD inline bool kin_bins_valid(const cuking_kin_bins &b) {
  return b.num_bins >= 1 && b.num_bins <= CUKING_KIN_BINS_MAX && kin_is_finite(b.lo) &&
         kin_is_finite(b.hi) && b.lo < b.hi;
}
// Once per call, on the host.
inline float kin_bin_scale(const cuking_kin_bins &b) { return (float)b.num_bins / (b.hi - b.lo); }
// The slot of `kin` (file header): THE definition.
CUKING_SUMMARY_HD inline uint32_t kin_bin_slot(float lo, float scale, uint32_t num_bins,
                                               float kin) {
  if (kin != kin) return num_bins + 2;  // NAN
  if (kin < lo) return 0;               // UNDER (-inf as well)
  const float t = (kin - lo) * scale;
  if (!(t < (float)num_bins)) return num_bins + 1;  // OVER (+inf, kin >= hi)
  return 1 + (uint32_t)t;
}

// ---- nearest-relative keys -------------------------------------------------------------
CUKING_SUMMARY_HD inline uint64_t kin_best_key(float kin, uint32_t partner) {
  if (kin != kin) return 0;
  const uint32_t b = kin_float_bits(kin);
  const uint32_t ordered = (b & 0x80000000u) ? ~b : (b ^ 0x80000000u);
  return ((uint64_t)ordered << 32) | (uint32_t)~partner;
}
// False for key 0 (nothing decoded).
CUKING_SUMMARY_HD inline bool kin_best_decode(uint64_t key, float *kin, uint32_t *partner) {
  if (key == 0) return false;
  const uint32_t ordered = (uint32_t)(key >> 32);
  *kin = kin_bits_float((ordered & 0x80000000u) ? (ordered ^ 0x80000000u) : ~ordered);
  *partner = ~(uint32_t)key;
  return true;
}

// ---- relative counts: bands ------------------------------------------------------------
constexpr uint32_t kRelNoBand = 0xFFFFFFFFu;
CUKING_SUMMARY_HD inline bool rel_thresholds_valid(const float *thresholds, uint32_t n) {
  if (thresholds == nullptr || n < 1 || n > CUKING_REL_THRESHOLDS_MAX) return false;
  for (uint32_t t = 0; t < n; ++t) {
    if (!kin_is_finite(thresholds[t])) return false;
    if (t != 0 && !(thresholds[t - 1] < thresholds[t])) return false;
  }
  return true;
}
// The band of `kin` (file header): THE definition.  (Ascending thresholds: the last one
// below kin is the largest.  A fixed trip count, unrolled on the device, so that thresholds
// held in registers are never indexed by a variable; entries from n on are not read.)
CUKING_SUMMARY_HD inline uint32_t rel_band(const float *thresholds, uint32_t n, float kin) {
  uint32_t band = kRelNoBand;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (uint32_t t = 0; t < CUKING_REL_THRESHOLDS_MAX; ++t)
    if (t < n && kin > thresholds[t]) band = t;
  return band;
}

}  // namespace cuking

#endif  // CUKING_AMD_KING_KIN_SUMMARY_H_
