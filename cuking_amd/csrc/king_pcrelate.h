// PC-Relate (include/cuking_amd.h, "PC-Relate"): the element functions the kernel of
// king_pcrelate.hip, the host twin of king_host.cc and the tests share, so that they cannot
// drift apart.  Plain C++: hipcc compiles the functions for the device, the sanitizer build of
// the tests (tests/pcrelate_host_driver.cc) for the host.  Neither build may contract a
// multiply and an add of these functions into one instruction (-ffp-contract=off); the only
// fused operations are the fmaf calls written out below.
//
// Element.  mu(i, s) = 0.5f * (fmaf chain in ascending c, from 0.0f, of X[i][c] * beta[s][c]),
// the individual-specific allele frequency of sample i at site s.  The element is VALID iff the
// genotype is called (geno_code != 3) and lo < mu < hi, both strict float32 comparisons.  Then
// r = (float)g - 2.0f * mu and v = sqrtf(mu * (1.0f - mu)) (correctly rounded); an invalid
// element has r = v = 0.0f.  Host and device hold the same r and v bit for bit.
//
// Sums.  num(i, j) = sum_s r(i, s) r(j, s), den(i, j) = sum_s v(i, s) v(j, s), kin = num /
// (4.0f * den) in IEEE float32 (NaN without a jointly valid site).  The zeros of the invalid
// elements are what restricts both sums to the jointly valid sites.
#ifndef CUKING_AMD_KING_PCRELATE_H_
#define CUKING_AMD_KING_PCRELATE_H_

#include <cmath>
#include <cstdint>

#include "king_geno.h"

namespace cuking {

// (CUKING_PCRELATE_COLUMNS_MAX)
constexpr uint32_t kPcrelateColumnsMax = 32;

// The fmaf chain over `d` columns; `D >= d` pads it with zero terms for callers whose rows are
// zero-padded registers (a zero term can only change the sign of a zero).
CUKING_HD inline float pcrelate_mu(const float *x_row, const float *beta_row, uint32_t d) {
  float acc = 0.0f;
  for (uint32_t c = 0; c < d; ++c) acc = fmaf(x_row[c], beta_row[c], acc);
  return 0.5f * acc;
}

CUKING_HD inline bool pcrelate_valid(uint32_t code, float mu, float lo, float hi) {
  return code != 3u && lo < mu && mu < hi;
}

// r and v of one element from its code and its mu.
CUKING_HD inline void pcrelate_element(uint32_t code, float mu, float lo, float hi, float *r,
                                       float *v) {
  const bool valid = pcrelate_valid(code, mu, lo, hi);
  const float twice = 2.0f * mu;
  const float var = mu * (1.0f - mu);
  *r = valid ? (float)code - twice : 0.0f;
  *v = valid ? sqrtf(var) : 0.0f;
}

CUKING_HD inline float pcrelate_kin(float num, float den) { return num / (4.0f * den); }

CUKING_HD inline bool pcrelate_bounds_valid(float lo, float hi) {
  return 0.0f <= lo && lo < hi && hi <= 1.0f;  // (false for a NaN)
}

}  // namespace cuking

#endif  // CUKING_AMD_KING_PCRELATE_H_
