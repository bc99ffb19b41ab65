// What the stand-alone sanitizer drivers (tests/*_host_driver.cc, built and run by
// tests/host_driver.py) share: the random numbers, the failure count and its two reporters, a bit
// of a word array and the genotype code of a site of a bitset row.  Every driver ends with the
// count print and `return g_failures != 0`.
#ifndef CUKING_AMD_TESTS_HOST_DRIVER_COMMON_H_
#define CUKING_AMD_TESTS_HOST_DRIVER_COMMON_H_

#include <cstdint>
#include <cstdio>

#include "cuking_amd.h"

inline uint64_t g_state = 0x9E3779B97F4A7C15ull;
inline uint64_t next_random() {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  uint64_t x = g_state;
  x ^= x >> 33;
  x *= 0xFF51AFD7ED558CCDull;
  x ^= x >> 33;
  return x;
}

inline int g_failures = 0;
// (a label and up to three numbers that place the failure: a shape, an index, a mode)
inline void fail(const char *what, uint64_t a = 0, uint64_t b = 0, uint64_t c = 0) {
  fprintf(stderr, "%s: %llu, %llu, %llu\n", what, (unsigned long long)a, (unsigned long long)b,
          (unsigned long long)c);
  ++g_failures;
}
inline void expect(const char *what, cuking_status got, cuking_status want) {
  if (got != want) {
    fprintf(stderr, "%s: status %d, expected %d (%s)\n", what, (int)got, (int)want,
            cuking_last_error());
    ++g_failures;
  }
}

inline bool bit_of(const uint64_t *words, uint64_t k) { return (words[k >> 6] >> (k & 63)) & 1; }

// 0 hom-ref, 1 het, 2 hom-var, 3 missing
inline uint32_t code_of(const uint64_t *row, uint32_t plane, uint32_t s) {
  return (uint32_t)((row[s >> 6] >> (s & 63)) & 1) |
         (uint32_t)((row[plane + (s >> 6)] >> (s & 63)) & 1) << 1;
}
inline void set_code(uint64_t *row, uint32_t plane, uint32_t s, uint32_t code) {
  const uint64_t bit = 1ull << (s & 63);
  row[s >> 6] = (row[s >> 6] & ~bit) | ((code & 1) ? bit : 0);
  row[plane + (s >> 6)] = (row[plane + (s >> 6)] & ~bit) | ((code & 2) ? bit : 0);
}

#endif  // CUKING_AMD_TESTS_HOST_DRIVER_COMMON_H_
