// LD pruning (include/cuking_amd.h, "LD pruning"): the definitions the kernels of king_ld.hip,
// the host functions of king_host.cc and the tests share, so that they cannot drift apart.
// Plain C++: hipcc compiles the functions for the device, the sanitizer build of the tests
// (tests/ld_host_driver.cc) for the host.
//
// Site-major bitset.  Q = ld_site_words(num_stored) = ceil(num_stored / 64); uint64
// site_bits[num_sites][2][Q], plane 0 = het, plane 1 = hom_var; sample s is bit s % 64 of word
// s / 64; missing is both bits set, as in the sample-major form.  Bits of samples >= num_stored
// in the last word are SET in both planes: the tail reads as missing.  Only real sites have
// rows.
//
// Per-pair sums.  For sites a < b, per site the masks N = ~(het & hom) (called), H = het &
// ~hom, V = hom & ~het (ld_masks); the dosage is g = H + 2 V.  With pc the popcount over all Q
// words, the nine counts of LdCounts give, over the samples called at both sites (ld_moments),
//     n = pc(Na & Nb)
//     Sx = pc(Ha & Nb) + 2 pc(Va & Nb)      Sxx = pc(Ha & Nb) + 4 pc(Va & Nb)
//     Sy, Syy likewise with a and b swapped
//     Sxy = pc(Ha & Hb) + 2 pc(Ha & Vb) + 2 pc(Va & Hb) + 4 pc(Va & Vb)
//     cov = n Sxy - Sx Sy      vx = n Sxx - Sx^2      vy = n Syy - Sy^2        (int64)
// num_stored is at most kLdMaxStored = 2^24: n Sxy <= 2^24 * 2^26 and Sx Sy <= 2^25 * 2^25,
// so every one of cov, vx, vy is an integer below 2^53 in magnitude and converts to double
// exactly.
//
// Edge rule.  (a, b) is an edge iff a < b < num_sites, b - a < window (a window of W variants:
// pairs up to W - 1 apart), group[a] == group[b] when groups are given, vx > 0, vy > 0 and
//     (double)cov * (double)cov > ((double)r2_threshold * (double)vx) * (double)vy
// (ld_is_edge): the float32 threshold promoted to double, three double products, each rounded
// once, no addition -- nothing a compiler could fuse, so host, device and a numpy restatement
// agree bit for bit.  Consequences: a monomorphic or all-missing site (vx = 0) has no edges;
// r2_threshold = 1 yields no edge at all (cov^2 <= vx vy by Cauchy-Schwarz, and for perfectly
// correlated sites both sides round the same integer); a NaN threshold, one outside [0, 1]
// (ld_threshold_valid) and window < 2 are refused.
//
// Edge record.  A cuking_result with sample_i = a, sample_j = b, kin = ld_r2 = (float)((double)
// cov * (double)cov / ((double)vx * (double)vy)), ibs0 = n, ibs1 = ibs2 = 0: exactly what
// cuking_unrelated_set consumes -- an edge list is a record buffer whose "samples" are sites.
//
// Default priority of a site (ld_priority), from its site_counts row (hom_ref, het, hom_var,
// missing) with called, alt and minor as cuking_site_mask_host defines them: (float)((double)
// minor / (double)(2 called)), NaN when called == 0, which unrel_key ranks last; among equal
// priorities the lower site index wins.
#ifndef CUKING_AMD_KING_LD_H_
#define CUKING_AMD_KING_LD_H_

#include <cstddef>
#include <cstdint>

#ifndef CUKING_HD
#ifdef __HIPCC__
#define CUKING_HD __host__ __device__
#else
#define CUKING_HD
#endif
#endif

namespace cuking {

constexpr uint32_t kLdMaxStored = 1u << 24;
// (what cuking_unrelated_set accepts: kUnrelMaxRecords)
constexpr uint64_t kLdMaxEdges = 1ull << 30;

CUKING_HD inline uint32_t ld_site_words(uint32_t num_stored) {
  return (uint32_t)(((uint64_t)num_stored + 63) / 64);
}
// (written so that NaN fails)
CUKING_HD inline bool ld_threshold_valid(float r2_threshold) {
  return r2_threshold >= 0.0f && r2_threshold <= 1.0f;
}
CUKING_HD inline bool ld_window_valid(uint32_t window) { return window >= 2; }

CUKING_HD inline void ld_masks(uint64_t het, uint64_t hom, uint64_t &n, uint64_t &h,
                               uint64_t &v) {
  n = ~(het & hom);
  h = het & ~hom;
  v = hom & ~het;
}

// The nine popcounts of a pair (a, b).
struct LdCounts {
  uint32_t nn;          // pc(Na & Nb)
  uint32_t hn, vn;      // pc(Ha & Nb), pc(Va & Nb)
  uint32_t nh, nv;      // pc(Na & Hb), pc(Na & Vb)
  uint32_t hh, hv, vh, vv;  // pc(Ha & Hb), pc(Ha & Vb), pc(Va & Hb), pc(Va & Vb)
  CUKING_HD void clear() { nn = hn = vn = nh = nv = hh = hv = vh = vv = 0; }
  // one word of both sites
  CUKING_HD void add(uint64_t na, uint64_t ha, uint64_t va, uint64_t nb, uint64_t hb,
                     uint64_t vb) {
    nn += (uint32_t)__builtin_popcountll(na & nb);
    hn += (uint32_t)__builtin_popcountll(ha & nb);
    vn += (uint32_t)__builtin_popcountll(va & nb);
    nh += (uint32_t)__builtin_popcountll(na & hb);
    nv += (uint32_t)__builtin_popcountll(na & vb);
    hh += (uint32_t)__builtin_popcountll(ha & hb);
    hv += (uint32_t)__builtin_popcountll(ha & vb);
    vh += (uint32_t)__builtin_popcountll(va & hb);
    vv += (uint32_t)__builtin_popcountll(va & vb);
  }
};

struct LdMoments {
  int64_t n, cov, vx, vy;
};

CUKING_HD inline LdMoments ld_moments(const LdCounts &c) {
  const int64_t n = c.nn;
  const int64_t sx = (int64_t)c.hn + 2 * (int64_t)c.vn, sxx = (int64_t)c.hn + 4 * (int64_t)c.vn;
  const int64_t sy = (int64_t)c.nh + 2 * (int64_t)c.nv, syy = (int64_t)c.nh + 4 * (int64_t)c.nv;
  const int64_t sxy = (int64_t)c.hh + 2 * (int64_t)c.hv + 2 * (int64_t)c.vh + 4 * (int64_t)c.vv;
  LdMoments m;
  m.n = n;
  m.cov = n * sxy - sx * sy;
  m.vx = n * sxx - sx * sx;
  m.vy = n * syy - sy * sy;
  return m;
}

// The part of the edge rule that needs the sums: THE comparison.
CUKING_HD inline bool ld_is_edge(const LdMoments &m, float r2_threshold) {
  if (!(m.vx > 0 && m.vy > 0)) return false;
  const double cov = (double)m.cov;
  const double lhs = cov * cov;
  const double scaled = (double)r2_threshold * (double)m.vx;
  const double rhs = scaled * (double)m.vy;
  return lhs > rhs;
}

// The r^2 an edge record carries (vx, vy > 0).
CUKING_HD inline float ld_r2(const LdMoments &m) {
  const double cov = (double)m.cov;
  const double num = cov * cov;
  const double den = (double)m.vx * (double)m.vy;
  return (float)(num / den);
}

// The part of the edge rule that needs no sums.
CUKING_HD inline bool ld_pair_in_band(uint64_t a, uint64_t b, uint32_t num_sites,
                                      uint32_t window) {
  return a < b && b < num_sites && b - a < window;
}

// The default priority of a site from its (hom_ref, het, hom_var, missing) counts.
CUKING_HD inline float ld_priority(const uint32_t counts[4]) {
  const uint64_t called = (uint64_t)counts[0] + counts[1] + counts[2];
  const uint64_t alt = (uint64_t)counts[1] + 2 * (uint64_t)counts[2];
  const uint64_t minor = alt < 2 * called - alt ? alt : 2 * called - alt;
  if (called == 0) return __builtin_nanf("");
  return (float)((double)minor / (double)(2 * called));
}

}  // namespace cuking

#endif  // CUKING_AMD_KING_LD_H_
