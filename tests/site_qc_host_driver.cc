// Stand-alone driver of the host side of site QC for the sanitizer build of
// tests/test_site_qc_host.py (built and run by tests/host_driver.py, csrc/king_host.cc linked in).
// Every buffer is an exact-size heap allocation, so a byte read or written past an end is caught.
//   1. cuking_compact_sites_host against a bit-by-bit restatement, over several shapes and masks;
//   2. the compaction kernel's own arithmetic (csrc/king_site_qc.h: the table built from the
//      mask, the walk that assembles one output word) run on the host against 1.;
//   3. cuking_site_mask_host on counts taken from the bitset, against the rule restated;
//   4. the bit-sliced counters of the count kernel (king_site_qc.h) over a full wavefront chunk
//      of all-ones and of random words, against plain sums.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "cuking_amd.h"
#include "host_driver_common.h"
#include "king_site_qc.h"

namespace {

// (fail: what, samples, sites, the kind of mask)

// a bitset as the pack leaves it: random codes, padding missing
std::unique_ptr<uint64_t[]> random_bitset(uint32_t n, uint32_t m, uint32_t wps) {
  std::unique_ptr<uint64_t[]> bits(new uint64_t[(size_t)n * wps]);
  const uint32_t plane = wps / 2;
  for (uint32_t s = 0; s < n; ++s)
    for (uint32_t w = 0; w < plane; ++w) {
      uint64_t het = next_random(), hom = next_random() & next_random();
      for (uint32_t b = 0; b < 64; ++b)
        if ((uint64_t)w * 64 + b >= m) {
          het |= 1ull << b;
          hom |= 1ull << b;
        }
      bits[(size_t)s * wps + w] = het;
      bits[(size_t)s * wps + plane + w] = hom;
    }
  return bits;
}

void make_mask(int kind, uint32_t m, uint32_t plane, uint64_t *keep) {
  memset(keep, 0, plane * 8);
  for (uint32_t s = 0; s < m; ++s) {
    bool k;
    switch (kind) {
      case 0: k = true; break;
      case 1: k = s == 0; break;
      case 2: k = s == m - 1; break;
      case 3: k = s & 1; break;
      case 4: k = next_random() % 50 == 0; break;
      case 5: k = next_random() % 2 == 0; break;
      case 6: k = next_random() % 50 != 0; break;
      default: k = (s >> 6) != 1 && (s >> 6) != 2; break;  // empty words between full ones
    }
    if (k) keep[s >> 6] |= 1ull << (s & 63);
  }
  bool any = false;
  for (uint32_t w = 0; w < plane; ++w) any |= keep[w] != 0;
  if (!any) keep[0] = 1;
}

void check_compaction(uint32_t n, uint32_t m, int kind) {
  const uint32_t wps = cuking_words_per_sample(m), plane = wps / 2;
  auto bits = random_bitset(n, m, wps);
  std::unique_ptr<uint64_t[]> keep(new uint64_t[plane]);
  make_mask(kind, m, plane, keep.get());
  uint32_t kept = 0;
  for (uint32_t s = 0; s < m; ++s) kept += bit_of(keep.get(), s);
  const uint32_t wps_out = cuking_words_per_sample(kept), plane_out = wps_out / 2;
  std::unique_ptr<uint64_t[]> got(new uint64_t[(size_t)n * wps_out]);
  memset(got.get(), 0xA5, (size_t)n * wps_out * 8);
  if (cuking_compact_sites_host(bits.get(), n, wps, keep.get(), m, got.get(), wps_out) !=
      CUKING_OK) {
    fprintf(stderr, "%s\n", cuking_last_error());
    return fail("compact_sites_host refused", n, m, kind);
  }
  // 1. bit by bit
  for (uint32_t s = 0; s < n; ++s) {
    const uint64_t *in = bits.get() + (size_t)s * wps, *out = got.get() + (size_t)s * wps_out;
    uint64_t k = 0;
    bool ok = true;
    for (uint32_t site = 0; site < m; ++site) {
      if (!bit_of(keep.get(), site)) continue;
      ok &= bit_of(out, k) == bit_of(in, site);
      ok &= bit_of(out + plane_out, k) == bit_of(in + plane, site);
      ++k;
    }
    for (; k < (uint64_t)plane_out * 64; ++k) ok &= bit_of(out, k) && bit_of(out + plane_out, k);
    if (!ok) return fail("compact_sites_host differs from the definition", n, m, kind);
  }
  // 2. the kernel's arithmetic
  const size_t table_bytes = cuking::compact_table_bytes(plane, plane_out);
  std::unique_ptr<uint64_t[]> table(new uint64_t[(table_bytes + 7) / 8]);
  if (cuking::build_compact_table(keep.get(), plane, plane_out, table.get()) != kept)
    return fail("build_compact_table counts another number of sites", n, m, kind);
  const cuking::CompactWord *words = reinterpret_cast<const cuking::CompactWord *>(table.get());
  const uint32_t *first_in = reinterpret_cast<const uint32_t *>(words + plane);
  for (uint32_t s0 = 0; s0 < n; s0 += cuking::kCompactRows) {
    const uint32_t rows = std::min(n - s0, cuking::kCompactRows);
    for (uint32_t j = 0; j < plane_out; ++j) {
      uint64_t het[cuking::kCompactRows], hom[cuking::kCompactRows];
      cuking::compact_output_word(words, first_in, plane, kept, bits.get() + (size_t)s0 * wps, wps,
                                  rows, j, het, hom);
      for (uint32_t r = 0; r < rows; ++r) {
        const uint64_t *out = got.get() + (size_t)(s0 + r) * wps_out;
        if (het[r] != out[j] || hom[r] != out[plane_out + j])
          return fail("compact_output_word differs from compact_sites_host", n, m, kind);
      }
    }
  }
  // 3. the site rule on this bitset's counts
  std::unique_ptr<uint32_t[]> counts(new uint32_t[(size_t)plane * 64 * 4]());
  for (uint32_t s = 0; s < n; ++s)
    for (uint64_t site = 0; site < (uint64_t)plane * 64; ++site) {
      const uint64_t *in = bits.get() + (size_t)s * wps;
      const int het = bit_of(in, site), hom = bit_of(in + plane, site);
      counts[site * 4 + (het && hom ? 3 : het ? 1 : hom ? 2 : 0)] += 1;
    }
  const cuking_site_filter rule = {0.9f, 0.05f, 2};
  std::unique_ptr<uint64_t[]> pass(new uint64_t[plane]);
  uint32_t passed = 0, expect = 0;
  if (cuking_site_mask_host(counts.get(), m, plane, &rule, keep.get(), pass.get(), &passed) !=
      CUKING_OK)
    return fail("site_mask_host refused", n, m, kind);
  for (uint64_t site = 0; site < (uint64_t)plane * 64; ++site) {
    const uint32_t *c = counts.get() + site * 4;
    const uint64_t called = (uint64_t)c[0] + c[1] + c[2], all = called + c[3];
    const uint64_t alt = c[1] + 2ull * c[2], minor = std::min(alt, 2 * called - alt);
    const bool want = site < m && called > 0 && (double)called >= (double)0.9f * (double)all &&
                      (double)minor >= (double)0.05f * (double)(2 * called) && minor >= 2 &&
                      bit_of(keep.get(), site);
    expect += want;
    if (want != bit_of(pass.get(), site)) return fail("site_mask_host differs", n, m, kind);
  }
  if (passed != expect) fail("site_mask_host counts another number of sites", n, m, kind);
}

void check_counters() {
  for (int ones = 0; ones < 2; ++ones) {
    cuking::SliceCounter counter;
    counter.clear();
    uint32_t want[64] = {};
    for (uint32_t s = 0; s < cuking::kSiteWaveSamples; s += cuking::kSiteGroup) {
      uint64_t x[cuking::kSiteGroup];
      for (uint32_t u = 0; u < cuking::kSiteGroup; ++u) {
        x[u] = ones ? ~0ull : next_random();
        for (uint32_t b = 0; b < 64; ++b) want[b] += (x[u] >> b) & 1;
      }
      counter.add8(x);
    }
    for (uint32_t b = 0; b < 64; ++b)
      if (counter.count(b >> 5, b & 31) != want[b]) {
        fprintf(stderr, "SliceCounter: bit %u holds %u, not %u (%s)\n", b,
                counter.count(b >> 5, b & 31), want[b], ones ? "all ones" : "random");
        ++g_failures;
      }
  }
}

}  // namespace

int main() {
  const uint32_t samples[] = {1, 3, 37, 65}, sites[] = {1, 31, 33, 63, 64, 65, 129, 700};
  for (uint32_t n : samples)
    for (uint32_t m : sites)
      for (int kind = 0; kind < 8; ++kind) check_compaction(n, m, kind);
  check_counters();
  // refusals leave the output alone
  {
    const uint32_t m = 129, wps = cuking_words_per_sample(m);
    auto bits = random_bitset(2, m, wps);
    std::unique_ptr<uint64_t[]> keep(new uint64_t[wps / 2]()), out(new uint64_t[2 * 2]);
    if (cuking_compact_sites_host(bits.get(), 2, wps, keep.get(), m, out.get(), 2) !=
            CUKING_ERR_INVALID_ARGUMENT ||
        strstr(cuking_last_error(), "no site passes") == nullptr)
      fail("an empty mask is not refused", 2, m);
    keep[2] = 2;  // site 129
    if (cuking_compact_sites_host(bits.get(), 2, wps, keep.get(), m, out.get(), 2) !=
        CUKING_ERR_INVALID_ARGUMENT)
      fail("a keep bit beyond num_sites is not refused", 2, m);
  }
  printf("site_qc_host_driver: %d failures\n", g_failures);
  return g_failures != 0;
}
