// PI_HAT, the method-of-moments IBD estimate of PLINK --genome and hl.identity_by_descent
// (include/cuking_amd.h, "PI_HAT (PLINK --genome)"): the definition the record epilogue of
// king_mfma.hip, the host twins of king_host.cc and the tests share, so that they cannot drift
// apart.  Plain C++: hipcc compiles the functions for the device, the sanitizer build of the
// tests (tests/pihat_host_driver.cc) for the host.
//
// ONE sequence of IEEE double operations -- only *, /, +, - and comparisons, in the order written
// below, every product and sum rounded on its own -- so that host, device and a restatement in any
// language with doubles agree bit for bit.  No multiply and add may be contracted into one
// instruction: both builds pass -ffp-contract=off, and the functions say so themselves where the
// compiler has a pragma for it.
//
// Model.  For a site with hom_ref = r, het = h, hom_var = v people (the order of site_counts):
// n = r + h + v, x = h + 2 v and y = h + 2 r allele counts, N = x + y.  F(a, k) = a (a - 1) ...
// (a - k + 1), multiplied left to right and 0 as soon as a factor is 0 (a monomorphic site needs
// no special case; no factor is ever negative).  A site is used iff n >= 2; its terms are the
// probabilities of drawing the alleles of two people without replacement (PLINK's finite-sample
// corrections written out):
//     a00 = (2 (F(x,2) F(y,2))) / F(N,4)
//     a01 = (4 (F(x,3) F(y,1) + F(x,1) F(y,3))) / F(N,4)
//     a02 = ((F(x,4) + F(y,4)) + 4 (F(x,2) F(y,2))) / F(N,4)
//     a11 = (2 (F(x,2) F(y,1) + F(x,1) F(y,2))) / F(N,3)
//     a12 = (((F(x,3) + F(y,3)) + F(x,2) F(y,1)) + F(x,1) F(y,2)) / F(N,3)
// E_uv = (sum of a_uv over the used sites, in site order) / sites_used.  No used site: NaN.
//
// Pair.  With S = ibs0 + ibs1 + ibs2 (exact):
//     z0 = ibs0 / (e00 S)
//     z1 = (ibs1 - z0 (e01 S)) / (e11 S)
//     z2 = ((ibs2 - z0 (e02 S)) - z1 (e12 S)) / S
// bounded (the default; PLINK without --nudge, Hail's bounded=True), in this order: z0 > 1 ->
// (1, 0, 0); z1 > 1 -> (0, 1, 0); z2 > 1 -> (0, 0, 1); z0 < 0 -> z0 = 0 and the other two divided
// by their sum; the same for z1 < 0; the same for z2 < 0.  pi_hat = z1 / 2 + z2.  Edges (S = 0, a
// zero expectation, NaN in the model) take whatever IEEE gives: every comparison with NaN is
// false, so NaN passes through the bounding and fails `> min_pi_hat`.  Where this differs from
// PLINK or Hail at such an edge, this text is the definition.
#ifndef CUKING_AMD_KING_PIHAT_H_
#define CUKING_AMD_KING_PIHAT_H_

#include <cstdint>

#include "cuking_amd.h"

#ifndef CUKING_HD
#ifdef __HIPCC__
#define CUKING_HD __host__ __device__
#else
#define CUKING_HD
#endif
#endif

#if defined(__clang__)
#define CUKING_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define CUKING_NO_CONTRACT  // (g++: -ffp-contract=off on the command line)
#endif

namespace cuking {

constexpr uint32_t kPihatMaxPeople = 1u << 24;
constexpr uint32_t kPihatUnbounded = 1u;  // CUKING_PIHAT_UNBOUNDED

// F(a, k), a a non-negative integer below 2^26 as a double.
CUKING_HD inline double pihat_falling(double a, int k) {
  CUKING_NO_CONTRACT
  double p = 1.0;
  for (int i = 0; i < k; ++i) {
    const double f = a - (double)i;
    if (f == 0.0) return 0.0;
    p = p * f;
  }
  return p;
}

// The five terms of one site (n >= 2, n <= kPihatMaxPeople): a00, a01, a02, a11, a12.
CUKING_HD inline void pihat_site_terms(uint32_t hom_ref, uint32_t het, uint32_t hom_var,
                                       double t[5]) {
  CUKING_NO_CONTRACT
  const double x = (double)((uint64_t)het + 2 * (uint64_t)hom_var);
  const double y = (double)((uint64_t)het + 2 * (uint64_t)hom_ref);
  const double N = x + y;
  const double x1 = pihat_falling(x, 1), x2 = pihat_falling(x, 2), x3 = pihat_falling(x, 3),
               x4 = pihat_falling(x, 4);
  const double y1 = pihat_falling(y, 1), y2 = pihat_falling(y, 2), y3 = pihat_falling(y, 3),
               y4 = pihat_falling(y, 4);
  const double n3 = pihat_falling(N, 3), n4 = pihat_falling(N, 4);
  const double x2y2 = x2 * y2, x3y1 = x3 * y1, x1y3 = x1 * y3, x2y1 = x2 * y1, x1y2 = x1 * y2;
  t[0] = (2.0 * x2y2) / n4;
  t[1] = (4.0 * (x3y1 + x1y3)) / n4;
  t[2] = ((x4 + y4) + 4.0 * x2y2) / n4;
  t[3] = (2.0 * (x2y1 + x1y2)) / n3;
  t[4] = (((x3 + y3) + x2y1) + x1y2) / n3;
}

// The model of num_sites count rows (uint32 [num_sites, 4]: hom_ref, het, hom_var, missing).
// False, and *bad_site set, when a row has more than kPihatMaxPeople people.
inline bool pihat_model_of_counts(const uint32_t *counts, uint32_t num_sites,
                                  cuking_pihat_model *model, uint32_t *bad_site) {
  CUKING_NO_CONTRACT
  double sum[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  uint32_t used = 0;
  for (uint32_t s = 0; s < num_sites; ++s) {
    const uint32_t *c = counts + (uint64_t)s * 4;
    const uint64_t n = (uint64_t)c[0] + c[1] + c[2];
    if (n > kPihatMaxPeople) {
      *bad_site = s;
      return false;
    }
    if (n < 2) continue;
    double t[5];
    pihat_site_terms(c[0], c[1], c[2], t);
    for (int k = 0; k < 5; ++k) sum[k] = sum[k] + t[k];
    ++used;
  }
  const double d = (double)used;
  model->e00 = sum[0] / d;
  model->e01 = sum[1] / d;
  model->e02 = sum[2] / d;
  model->e11 = sum[3] / d;
  model->e12 = sum[4] / d;
  model->sites_used = used;
  return true;
}

// z0, z1, z2, pi_hat of a pair's IBS counts.
CUKING_HD inline void pihat_z_of_counts(double e00, double e01, double e02, double e11,
                                        double e12, uint32_t ibs0, uint32_t ibs1, uint32_t ibs2,
                                        bool bounded, double z[4]) {
  CUKING_NO_CONTRACT
  const double S = ((double)ibs0 + (double)ibs1) + (double)ibs2;
  double z0 = (double)ibs0 / (e00 * S);
  double z1 = ((double)ibs1 - z0 * (e01 * S)) / (e11 * S);
  double z2 = (((double)ibs2 - z0 * (e02 * S)) - z1 * (e12 * S)) / S;
  if (bounded) {
    if (z0 > 1.0) {
      z0 = 1.0;
      z1 = 0.0;
      z2 = 0.0;
    }
    if (z1 > 1.0) {
      z0 = 0.0;
      z1 = 1.0;
      z2 = 0.0;
    }
    if (z2 > 1.0) {
      z0 = 0.0;
      z1 = 0.0;
      z2 = 1.0;
    }
    if (z0 < 0.0) {
      const double s = z1 + z2;
      z0 = 0.0;
      z1 = z1 / s;
      z2 = z2 / s;
    }
    if (z1 < 0.0) {
      const double s = z0 + z2;
      z1 = 0.0;
      z0 = z0 / s;
      z2 = z2 / s;
    }
    if (z2 < 0.0) {
      const double s = z0 + z1;
      z2 = 0.0;
      z0 = z0 / s;
      z1 = z1 / s;
    }
  }
  z[0] = z0;
  z[1] = z1;
  z[2] = z2;
  z[3] = z1 / 2.0 + z2;
}

// What a record carries and the scan decides on: (float)pi_hat.
CUKING_HD inline float pihat_of_counts(double e00, double e01, double e02, double e11, double e12,
                                       uint32_t ibs0, uint32_t ibs1, uint32_t ibs2,
                                       uint32_t flags) {
  double z[4];
  pihat_z_of_counts(e00, e01, e02, e11, e12, ibs0, ibs1, ibs2, (flags & kPihatUnbounded) == 0, z);
  return (float)z[3];
}

}  // namespace cuking

#endif  // CUKING_AMD_KING_PIHAT_H_
