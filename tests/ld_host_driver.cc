// Stand-alone driver of the host side of LD pruning for the sanitizer build of
// tests/test_ld_host.py (built and run by tests/host_driver.py, csrc/king_host.cc linked in).
// Every buffer is an exact-size heap allocation, so a byte read or written past an end is caught.
//   1. cuking_transpose_sites_host against a bit-by-bit restatement, over the odd shapes;
//   2. cuking_ld_edges_host against the sums taken from plain genotype arrays and the
//      comparison of csrc/king_ld.h, with and without groups, and its overflow path;
//   3. the helpers of king_ld.h: masks, counts and moments of random words against sums over
//      the bits, the threshold and window rules, the priority.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "cuking_amd.h"
#include "host_driver_common.h"
#include "king_ld.h"

namespace {

// (fail: what, samples, sites, window)

// genotypes [n][m]: 0, 1, 2 or -1 (missing); a site copies its left neighbour now and then
std::vector<int8_t> random_genotypes(uint32_t n, uint32_t m) {
  std::vector<int8_t> g((size_t)n * m);
  for (uint32_t s = 0; s < n; ++s)
    for (uint32_t k = 0; k < m; ++k) {
      const uint64_t r = next_random();
      int8_t v = (int8_t)((r & 3) == 3 ? -1 : (r & 3));
      if (k % 5 && ((r >> 8) & 3)) v = g[(size_t)s * m + k - 1];
      g[(size_t)s * m + k] = v;
    }
  return g;
}

void run_shape(uint32_t n, uint32_t m) {
  const std::vector<int8_t> g = random_genotypes(n, m);
  const uint32_t wps = cuking_words_per_sample(m), plane = wps / 2, q = cuking::ld_site_words(n);
  std::unique_ptr<uint64_t[]> bits(new uint64_t[(size_t)n * wps]);
  for (size_t k = 0; k < (size_t)n * wps; ++k) bits[k] = ~0ull;  // padding: missing
  for (uint32_t s = 0; s < n; ++s)
    for (uint32_t k = 0; k < m; ++k) {
      const int8_t v = g[(size_t)s * m + k];
      if (v != 1 && v >= 0) bits[(size_t)s * wps + k / 64] &= ~(1ull << (k % 64));
      if (v != 2 && v >= 0) bits[(size_t)s * wps + plane + k / 64] &= ~(1ull << (k % 64));
    }
  std::unique_ptr<uint64_t[]> site_bits(new uint64_t[(size_t)m * 2 * q]);
  if (cuking_transpose_sites_host(bits.get(), n, wps, m, site_bits.get(), q) != CUKING_OK)
    return fail("transpose refused", n, m, 0);
  for (uint32_t k = 0; k < m; ++k)
    for (uint32_t s = 0; s < 64 * q; ++s) {
      const int8_t v = s < n ? g[(size_t)s * m + k] : (int8_t)-1;
      const bool het = (site_bits[((size_t)k * 2) * q + s / 64] >> (s % 64)) & 1;
      const bool hom = (site_bits[((size_t)k * 2 + 1) * q + s / 64] >> (s % 64)) & 1;
      if (het != (v == 1 || v < 0) || hom != (v == 2 || v < 0)) return fail("transpose", n, m, 0);
    }
  std::unique_ptr<int32_t[]> group(new int32_t[m]);
  for (uint32_t k = 0; k < m; ++k) group[k] = (int32_t)(k / 37);
  const uint32_t windows[] = {2, 7, 64, 65, m + 10};
  const float thresholds[] = {0.0f, 0.2f, 0.999f, 1.0f};
  for (const uint32_t window : windows)
    for (const float thr : thresholds)
      for (int grouped = 0; grouped < 2; ++grouped) {
        std::vector<cuking_result> want;
        for (uint32_t a = 0; a < m; ++a)
          for (uint32_t b = a + 1; b < m && b - a < window; ++b) {
            if (grouped && group[a] != group[b]) continue;
            int64_t cnt = 0, sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
            for (uint32_t s = 0; s < n; ++s) {
              const int64_t x = g[(size_t)s * m + a], y = g[(size_t)s * m + b];
              if (x < 0 || y < 0) continue;
              ++cnt, sx += x, sy += y, sxx += x * x, syy += y * y, sxy += x * y;
            }
            const cuking::LdMoments mo{cnt, cnt * sxy - sx * sy, cnt * sxx - sx * sx,
                                       cnt * syy - sy * sy};
            if (cuking::ld_is_edge(mo, thr))
              want.push_back(cuking_result{a, b, cuking::ld_r2(mo), (uint32_t)cnt, 0, 0});
          }
        if (thr == 1.0f && !want.empty()) fail("an edge at threshold 1", n, m, window);
        uint64_t count = ~0ull;
        std::unique_ptr<cuking_result[]> got(new cuking_result[want.size()]);
        const cuking_status st =
            cuking_ld_edges_host(site_bits.get(), m, n, window, thr, grouped ? group.get() : nullptr,
                                 want.empty() ? nullptr : got.get(), want.size(), &count);
        if (st != CUKING_OK || count != want.size()) {
          fail("edge count", n, m, window);
          continue;
        }
        for (size_t k = 0; k < want.size(); ++k)  // (the host function walks in (a, b) order)
          if (got[k].sample_i != want[k].sample_i || got[k].sample_j != want[k].sample_j ||
              got[k].kin != want[k].kin || got[k].ibs0 != want[k].ibs0 || got[k].ibs1 != 0 ||
              got[k].ibs2 != 0) {
            fail("edge record", n, m, window);
            break;
          }
        if (want.size() > 1) {  // one record short: the exact count, nothing past the buffer
          std::unique_ptr<cuking_result[]> tight(new cuking_result[want.size() - 1]);
          if (cuking_ld_edges_host(site_bits.get(), m, n, window, thr,
                                   grouped ? group.get() : nullptr, tight.get(), want.size() - 1,
                                   &count) != CUKING_ERR_RESOURCE_EXHAUSTED ||
              count != want.size())
            fail("overflow", n, m, window);
        }
      }
}

void check_helpers() {
  for (int round = 0; round < 2000; ++round) {
    const uint64_t a_het = next_random(), a_hom = next_random(), b_het = next_random(),
                   b_hom = next_random();
    uint64_t na, ha, va, nb, hb, vb;
    cuking::ld_masks(a_het, a_hom, na, ha, va);
    cuking::ld_masks(b_het, b_hom, nb, hb, vb);
    cuking::LdCounts c;
    c.clear();
    c.add(na, ha, va, nb, hb, vb);
    int64_t n = 0, sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
    for (int bit = 0; bit < 64; ++bit) {
      const int ah = (a_het >> bit) & 1, am = (a_hom >> bit) & 1;
      const int bh = (b_het >> bit) & 1, bm = (b_hom >> bit) & 1;
      if ((ah && am) || (bh && bm)) continue;
      const int64_t x = ah + 2 * am, y = bh + 2 * bm;
      ++n, sx += x, sy += y, sxx += x * x, syy += y * y, sxy += x * y;
    }
    const cuking::LdMoments m = cuking::ld_moments(c);
    if (m.n != n || m.cov != n * sxy - sx * sy || m.vx != n * sxx - sx * sx ||
        m.vy != n * syy - sy * sy)
      fail("moments", 64, 2, 0);
  }
  // the largest sums a call may meet: 2^24 samples, all hom-var against half hom-var
  cuking::LdCounts big;
  big.clear();
  big.nn = 1u << 24;
  big.vn = 1u << 24;
  big.nv = 1u << 23;
  big.vv = 1u << 23;
  const cuking::LdMoments m = cuking::ld_moments(big);
  if (m.vx != 0 || m.vy <= 0 || m.vy >= (1ll << 53) || cuking::ld_is_edge(m, 0.0f))
    fail("largest sums", 1u << 24, 2, 0);
  if (cuking::ld_threshold_valid(NAN) || cuking::ld_threshold_valid(-0.5f) ||
      cuking::ld_threshold_valid(1.5f) || !cuking::ld_threshold_valid(0.0f) ||
      !cuking::ld_threshold_valid(1.0f) || cuking::ld_window_valid(0) ||
      cuking::ld_window_valid(1) || !cuking::ld_window_valid(2))
    fail("argument rules", 0, 0, 0);
  const uint32_t none[4] = {0, 0, 0, 5}, some[4] = {6, 1, 1, 2};
  if (!std::isnan(cuking_ld_priority(none)) || cuking_ld_priority(some) != (float)(3.0 / 16.0))
    fail("priority", 0, 0, 0);
  if (cuking::ld_site_words(0) != 0 || cuking::ld_site_words(64) != 1 ||
      cuking::ld_site_words(65) != 2 || cuking::ld_site_words(0xFFFFFFFFu) != (1u << 26))
    fail("site words", 0, 0, 0);
}

}  // namespace

int main() {
  const uint32_t samples[] = {1, 63, 64, 65, 130}, sites[] = {1, 64, 65, 150};
  for (const uint32_t n : samples)
    for (const uint32_t m : sites) run_shape(n, m);
  check_helpers();
  printf("%d failures\n", g_failures);
  return g_failures != 0;
}
