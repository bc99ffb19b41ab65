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
//
// Records (include/cuking_amd.h, "PC-Relate records"; king_pcrelate_records.hip and
// cuking_pcrelate_records_host).  The same sums and kin -- on the device the matrix and the
// record kernel call one tile body, king_pcrelate_tile.h --; pcrelate_is_record is the rule that
// makes a pair a record, pcrelate_triangle_tile the map from a workgroup's number to its tile
// when only the upper triangle of a diagonal block is launched.
//
// Listed pairs (include/cuking_amd.h, "PC-Relate for listed pairs"; king_pcrelate_pairs.hip and
// cuking_pcrelate_pairs_host).  On top of the element above, with f the sample's inbreeding
// coefficient: var = mu * (1.0f - mu), s2 = (1.0f + f) * var, dom = mu, 0.0f or 1.0f - mu for
// the codes 0, 1, 2, e = dom - s2; an invalid element has s2 = e = 0.0f.  A pair holds seven
// sums over its jointly valid sites (PcrelatePairSums); each float sum is ONE float32 chain from
// +0.0f in ascending s with one fmaf per term, which pcrelate_pair_site writes out and host and
// device both run, so the two agree bit for bit.  pcrelate_pair_result turns the sums into kin,
// k0, k1, k2.
#ifndef CUKING_AMD_KING_PCRELATE_H_
#define CUKING_AMD_KING_PCRELATE_H_

#include <cmath>
#include <cstdint>
#include <type_traits>

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

#ifdef __HIPCC__
// The kernels hold an X row in D registers, D = d rounded up to 4 / 8 / 16 / 32, a template
// parameter: `launch(std::integral_constant<uint32_t, D>)` launches the kernel for that D.
template <typename Launch>
hipError_t pcrelate_dispatch_columns(uint32_t d, Launch &&launch) {
  if (d <= 4) return launch(std::integral_constant<uint32_t, 4>{});
  if (d <= 8) return launch(std::integral_constant<uint32_t, 8>{});
  if (d <= 16) return launch(std::integral_constant<uint32_t, 16>{});
  return launch(std::integral_constant<uint32_t, kPcrelateColumnsMax>{});
}
#endif

// ---- records (include/cuking_amd.h, "PC-Relate records") -------------------------------------

// A pair is a record iff its kinship is above the threshold: the strict float32 comparison of
// a KING record, false for a NaN on either side.
CUKING_HD inline bool pcrelate_is_record(float kin, float min_kin) { return kin > min_kin; }

// Tiles of a diagonal block of `side` x `side` tiles: the upper triangle with its diagonal,
// tile_j >= tile_i, numbered row by row -- row i holds side - i tiles and starts at
// i side - i (i - 1) / 2.  side <= 2^25 (2^32 - 1 samples in tiles of 128), so every count is
// below 2^50.
constexpr uint64_t kPcrelateTriangleSideMax = 1ull << 25;  // (CUKING_PCRELATE_TRIANGLE_SIDE_MAX)

CUKING_HD inline uint64_t pcrelate_triangle_tiles(uint64_t side) { return side * (side + 1) / 2; }

CUKING_HD inline uint64_t pcrelate_triangle_index(uint64_t side, uint32_t tile_i, uint32_t tile_j) {
  const uint64_t i = tile_i;
  return i * (2 * side - i + 1) / 2 + (tile_j - i);  // (one of the two factors is even)
}

// The inverse.  Counted from the END, the triangle is rows of 1, 2, 3, ... tiles: `back` tiles
// behind `index` put it into row m from the end, m the largest with m (m + 1) / 2 <= back.  The
// square root (8 back + 1 < 2^53 is exact in a double) only proposes m; the two loops make it
// exact whatever the rounding of sqrt.
CUKING_HD inline void pcrelate_triangle_tile(uint64_t side, uint64_t index, uint32_t *tile_i,
                                             uint32_t *tile_j) {
  const uint64_t back = pcrelate_triangle_tiles(side) - 1 - index;
  uint64_t m = (uint64_t)((sqrt((double)(8 * back + 1)) - 1.0) * 0.5);
  while (m * (m + 1) / 2 > back) --m;
  while ((m + 1) * (m + 2) / 2 <= back) ++m;
  *tile_i = (uint32_t)(side - 1 - m);
  *tile_j = (uint32_t)(side - 1 - (back - m * (m + 1) / 2));
}

// ---- listed pairs ----------------------------------------------------------------------------

// (CUKING_PCRELATE_K0_SWITCH: 2^(-5/2) rounded to float32, 0x3E3504F3)
constexpr float kPcrelateK0Switch = 0.17677669529663689f;

// s2 and e of one element; `one_plus_f` = 1.0f + f of its sample.
CUKING_HD inline void pcrelate_dominance(uint32_t code, float mu, bool valid, float one_plus_f,
                                         float *s2, float *e) {
  const float var = mu * (1.0f - mu);
  const float scaled = one_plus_f * var;
  const float dom = code == 0u ? mu : code == 1u ? 0.0f : 1.0f - mu;
  const float diff = dom - scaled;
  *s2 = valid ? scaled : 0.0f;
  *e = valid ? diff : 0.0f;
}

struct PcrelatePairSums {
  float num = 0.0f, den = 0.0f, dnum = 0.0f, dden = 0.0f, hden = 0.0f;
  uint32_t ibs0 = 0, sites = 0;
};

// One site of one pair: i is the first sample of the chains, j the second (the callers put the
// smaller index first, which is what makes (i, j) and (j, i) the same bytes although the two
// terms of hden are taken in a fixed order).  A site that is not jointly valid adds nothing.
CUKING_HD inline void pcrelate_pair_site(PcrelatePairSums *sum, uint32_t code_i, float mu_i,
                                         float one_plus_f_i, uint32_t code_j, float mu_j,
                                         float one_plus_f_j, float lo, float hi) {
  float r_i, v_i, s2_i, e_i, r_j, v_j, s2_j, e_j;
  const bool valid_i = pcrelate_valid(code_i, mu_i, lo, hi);
  const bool valid_j = pcrelate_valid(code_j, mu_j, lo, hi);
  pcrelate_element(code_i, mu_i, lo, hi, &r_i, &v_i);
  pcrelate_element(code_j, mu_j, lo, hi, &r_j, &v_j);
  pcrelate_dominance(code_i, mu_i, valid_i, one_plus_f_i, &s2_i, &e_i);
  pcrelate_dominance(code_j, mu_j, valid_j, one_plus_f_j, &s2_j, &e_j);
  const float a = mu_i * (1.0f - mu_j);
  const float b = (1.0f - mu_i) * mu_j;
  const float num = fmaf(r_i, r_j, sum->num);
  const float den = fmaf(v_i, v_j, sum->den);
  const float dnum = fmaf(e_i, e_j, sum->dnum);
  const float dden = fmaf(s2_i, s2_j, sum->dden);
  const float hden = fmaf(b, b, fmaf(a, a, sum->hden));
  const bool joint = valid_i && valid_j;
  sum->num = joint ? num : sum->num;
  sum->den = joint ? den : sum->den;
  sum->dnum = joint ? dnum : sum->dnum;
  sum->dden = joint ? dden : sum->dden;
  sum->hden = joint ? hden : sum->hden;
  // (jointly valid codes are 0, 1, 2: only (0, 2) and (2, 0) differ in exactly the hom bit)
  sum->ibs0 += (joint && (code_i ^ code_j) == 2u) ? 1u : 0u;
  sum->sites += joint ? 1u : 0u;
}

// Every NaN is stored as the one quiet NaN 0x7FC00000, whatever the division made of it.
CUKING_HD inline float pcrelate_canonical(float value) {
  return value != value ? __builtin_nanf("") : value;
}

CUKING_HD inline void pcrelate_pair_result(const PcrelatePairSums &sum, float *kin, float *k0,
                                           float *k1, float *k2) {
  const float kin_v = pcrelate_kin(sum.num, sum.den);
  const float k2_v = sum.dnum / sum.dden;
  const float high = (1.0f - 4.0f * kin_v) + k2_v;
  const float low = (float)sum.ibs0 / sum.hden;
  const float k0_v = kin_v > kPcrelateK0Switch ? high : low;   // (false for a NaN)
  const float k1_v = (1.0f - k2_v) - k0_v;
  *kin = pcrelate_canonical(kin_v);
  *k0 = pcrelate_canonical(k0_v);
  *k1 = pcrelate_canonical(k1_v);
  *k2 = pcrelate_canonical(k2_v);
}

CUKING_HD inline bool pcrelate_pair_stride_valid(uint32_t pair_stride) {
  return pair_stride >= 8u && pair_stride % 4u == 0u;
}

}  // namespace cuking

#endif  // CUKING_AMD_KING_PCRELATE_H_
