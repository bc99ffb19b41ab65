// Stand-alone driver of the Hardy-Weinberg host twin for the sanitizer build of
// tests/test_hwe_host.py (built and run by tests/host_driver.py, csrc/king_host.cc linked in): a
// program of its own, nothing is loaded into Python.
//
// Reads count rows "hom_ref het hom_var" from standard input, one per line, and for every row
// prints the bits of four doubles in hex: hwe_exact_p (csrc/king_hwe.h) without and with mid-p,
// then cuking_hwe_sites_host (csrc/king_host.cc) on the whole array without and with
// CUKING_HWE_MIDP.  The arrays are heap blocks of exactly the size the contract names, so a read
// of row num_sites or a store past p[num_sites - 1] is a sanitizer report.  Then the refusals.
// Ends with "<n> failures".
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cuking_amd.h"
#include "host_driver_common.h"
#include "king_hwe.h"

#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      ++g_failures;                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
    }                                                                  \
  } while (0)

static uint64_t bits_of(double x) {
  uint64_t b;
  std::memcpy(&b, &x, sizeof b);
  return b;
}

int main() {
  std::vector<uint32_t> rows;
  unsigned long long a, b, c;
  while (std::scanf("%llu %llu %llu", &a, &b, &c) == 3) {
    rows.push_back((uint32_t)a);
    rows.push_back((uint32_t)b);
    rows.push_back((uint32_t)c);
  }
  const uint32_t n = (uint32_t)(rows.size() / 3);
  // exactly n rows of four and n doubles, on the heap
  uint32_t *counts = new uint32_t[(size_t)n * 4];
  double *p = new double[n], *p_mid = new double[n];
  for (uint32_t s = 0; s < n; ++s) {
    counts[4 * s + 0] = rows[3 * s + 0];
    counts[4 * s + 1] = rows[3 * s + 1];
    counts[4 * s + 2] = rows[3 * s + 2];
    counts[4 * s + 3] = 0xDEADBEEFu + s;  // missing: ignored
  }
  EXPECT(cuking_hwe_sites_host(counts, n, 0, p) == CUKING_OK);
  EXPECT(cuking_hwe_sites_host(counts, n, CUKING_HWE_MIDP, p_mid) == CUKING_OK);
  for (uint32_t s = 0; s < n; ++s) {
    const double direct = cuking::hwe_exact_p(rows[3 * s], rows[3 * s + 1], rows[3 * s + 2], false);
    const double direct_mid =
        cuking::hwe_exact_p(rows[3 * s], rows[3 * s + 1], rows[3 * s + 2], true);
    std::printf("row %u %u %u: %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n",
                rows[3 * s], rows[3 * s + 1], rows[3 * s + 2], bits_of(direct),
                bits_of(direct_mid), bits_of(p[s]), bits_of(p_mid[s]));
  }

  // refusals, and what is no work
  EXPECT(cuking_hwe_sites_host(counts, n, 2, p) == CUKING_ERR_INVALID_ARGUMENT);
  EXPECT(cuking_hwe_sites_host(counts, n, 0x80000001u, p) == CUKING_ERR_INVALID_ARGUMENT);
  EXPECT(cuking_hwe_sites_host(nullptr, 0, 2, nullptr) == CUKING_ERR_INVALID_ARGUMENT);
  if (n != 0) {
    EXPECT(cuking_hwe_sites_host(nullptr, n, 0, p) == CUKING_ERR_INVALID_ARGUMENT);
    EXPECT(cuking_hwe_sites_host(counts, n, 0, nullptr) == CUKING_ERR_INVALID_ARGUMENT);
  }
  if (n > 1) {
    // a shorter call leaves the rest alone
    const double before = p[n - 1];
    p[0] = -1.0;
    EXPECT(cuking_hwe_sites_host(counts, 1, 0, p) == CUKING_OK);
    EXPECT(p[0] != -1.0 && bits_of(p[n - 1]) == bits_of(before));
  }
  EXPECT(cuking_hwe_sites_host(nullptr, 0, 0, nullptr) == CUKING_OK);
  EXPECT(cuking_hwe_sites_host(nullptr, 0, CUKING_HWE_MIDP, nullptr) == CUKING_OK);

  delete[] counts;
  delete[] p;
  delete[] p_mid;
  std::printf("%d failures\n", g_failures);
  return g_failures != 0;
}
