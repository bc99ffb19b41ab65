// Hardy-Weinberg exact test per site (include/cuking_amd.h, "Hardy-Weinberg test"): the
// definition the kernel of king_hwe.hip, the host twin of king_host.cc and the tests share, so
// that they cannot drift apart.  Plain C++: hipcc compiles the function for the device, the
// sanitizer build of the tests (tests/hwe_host_driver.cc) for the host.
//
// The test of Wigginton, Cutler and Abecasis (2005), walked array-free from the observed table
// outward.  With n = hom_ref + het + hom_var people and the rare homozygote count r0 = min(hom_ref,
// hom_var), c0 = max(hom_ref, hom_var), the tables with the observed allele counts are those with
// het + 2 k heterozygotes, k = -floor(het / 2) .. r0, and the probability of a table relative to
// its neighbour with two heterozygotes less, (x, hr, hc) -> (x + 2, hr - 1, hc - 1), is
//     4 hr hc / ((x + 2) (x + 1)).
// The observed table is term 1.0; `total` is the sum of all terms, `tail` that of the terms no
// larger than the observed one (itself included), and p = tail / total.  With `midp` half the
// observed table's term leaves the tail (Graffelman and Moreno 2013).
//
// ONE sequence of IEEE double operations, so that host, device and a restatement in any language
// with doubles agree bit for bit: up first, then down; t = (t * num) / den with the two integer
// products num and den formed first (both below 2^50: exact); total and tail grow in walk order.
// Subnormal terms are kept (no flush to zero anywhere); a term that underflows to 0.0 ends its
// direction, because every later term of that direction is smaller; a term that overflows (the
// observed table is more than 10^308 times less likely than another) makes p = 0.0.
//
// kHweTie = 1 + 2^-27 is derived, not tuned: a table exactly as likely as the observed one is
// reached after at most 2^24 steps of two roundings each, so its computed term is within
// 2 * 2^24 * 2^-53 = 2^-28 of 1, and with this constant every exact tie is counted whatever
// n <= 2^24 is.  n = 0 gives 1.0, n > kHweMaxPeople = 2^24 (the library's sample limit) NaN.
#ifndef CUKING_AMD_KING_HWE_H_
#define CUKING_AMD_KING_HWE_H_

#include <cstdint>

#ifndef CUKING_HD
#ifdef __HIPCC__
#define CUKING_HD __host__ __device__
#else
#define CUKING_HD
#endif
#endif

namespace cuking {

constexpr uint32_t kHweMaxPeople = 1u << 24;
constexpr double kHweTie = 1.0 + 0x1p-27;
constexpr uint32_t kHweMidp = 1u;  // CUKING_HWE_MIDP

CUKING_HD inline double hwe_exact_p(uint32_t hom_ref, uint32_t het, uint32_t hom_var, bool midp) {
  const uint64_t n = (uint64_t)hom_ref + het + hom_var;
  if (n == 0) return 1.0;
  if (n > kHweMaxPeople) return __builtin_nan("");
  const double r0 = (double)(hom_ref < hom_var ? hom_ref : hom_var);
  const double c0 = (double)(hom_ref < hom_var ? hom_var : hom_ref);
  const double inf = __builtin_inf();
  double total = 1.0, tail = 1.0;
  // up: more heterozygotes
  double t = 1.0, x = (double)het, hr = r0, hc = c0;
  while (hr > 0.0) {
    const double num = 4.0 * hr * hc;
    const double den = (x + 2.0) * (x + 1.0);
    t = (t * num) / den;
    x += 2.0;
    hr -= 1.0;
    hc -= 1.0;
    if (t == 0.0) break;
    if (!(t < inf)) return 0.0;
    total += t;
    if (t <= kHweTie) tail += t;
  }
  // down: fewer heterozygotes
  t = 1.0;
  x = (double)het;
  hr = r0;
  hc = c0;
  while (x >= 2.0) {
    const double num = x * (x - 1.0);
    const double den = 4.0 * (hr + 1.0) * (hc + 1.0);
    t = (t * num) / den;
    x -= 2.0;
    hr += 1.0;
    hc += 1.0;
    if (t == 0.0) break;
    if (!(t < inf)) return 0.0;
    total += t;
    if (t <= kHweTie) tail += t;
  }
  if (midp) tail -= 0.5;
  return tail / total;
}

}  // namespace cuking

#endif  // CUKING_AMD_KING_HWE_H_
