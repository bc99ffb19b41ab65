// Stand-alone driver of the host side of the Mendelian errors for the sanitizer build of
// tests/test_mendel_host.py (built and run by tests/host_driver.py, csrc/king_host.cc linked in).
// Every buffer is an exact-size heap allocation, so a byte read or written past an end is caught
// -- the planes of exactly ceil(num_sites / 64) words, the list of trios, the rows, the mask and
// the counts above all.
//   1. mendel_code_masks on random words: the eight masks are pairwise disjoint, with and without
//      absent parents;
//   2. cuking_mendel_trios_host and cuking_mendel_site_counts_host against a walk over the sites one
//      by one, for full trios, duos, absent and out-of-range samples and repeats, with random bits
//      beyond num_sites; with and without the mask; the counts accumulate over two calls;
//   3. the refusals, which write nothing.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "cuking_amd.h"
#include "host_driver_common.h"
#include "king_mendel.h"

namespace {

// (fail: what, sites, one more number)

// The table of the header, written out: the error code of one site, 0 for none.
uint32_t classify(uint32_t f, uint32_t m, uint32_t c) {
  if (c == 1) return f == 0 && m == 0 ? 1 : f == 2 && m == 2 ? 2 : 0;
  if (c == 0) return f == 2 && m == 2 ? 5 : f == 2 ? 3 : m == 2 ? 4 : 0;
  if (c == 2) return f == 0 && m == 0 ? 8 : f == 0 ? 6 : m == 0 ? 7 : 0;
  return 0;
}

void check_disjoint() {
  for (int round = 0; round < 2000; ++round) {
    const uint64_t valid = round % 3 == 0 ? ~0ull : next_random();
    cuking::MendelWord x[3];
    for (int k = 0; k < 3; ++k) x[k] = cuking::mendel_word(next_random(), next_random(), valid);
    if (round % 5 == 1) x[1] = cuking::MendelWord();
    if (round % 7 == 2) x[2] = cuking::MendelWord();
    uint64_t code[cuking::kMendelCodes];
    cuking::mendel_code_masks(x[1], x[2], x[0], code);
    for (uint32_t a = 0; a < cuking::kMendelCodes; ++a) {
      if (code[a] & ~valid) fail("a code outside the valid sites", 64, a);
      for (uint32_t b = a + 1; b < cuking::kMendelCodes; ++b)
        if (code[a] & code[b]) fail("two codes at one site", 64, a * 8 + b);
    }
  }
}

void run_shape(uint32_t sites, uint32_t n, bool with_mask) {
  const uint32_t plane = (sites + 63) / 64 ? (sites + 63) / 64 : 1, words = 2 * plane;
  std::unique_ptr<uint64_t[]> bits(new uint64_t[(size_t)n * words]);
  for (size_t k = 0; k < (size_t)n * words; ++k) bits[k] = next_random() & next_random();
  const uint32_t none = CUKING_MENDEL_NO_PARENT;
  std::vector<uint32_t> list = {0, 1, 2,    3 % n, 1, 2,    0, 1, none, 0, none, 2,
                                0, none, none, 0, 1, 2, 1, n,    2,    1, 0, n + 5,
                                n, 0,    1,    2, 2, 1};
  // (with few samples some of these lie beyond the stored ones: legal, and missing everywhere)
  for (int k = 0; k < 12; ++k) list.push_back((uint32_t)(next_random() % (n + 1)));
  const uint64_t num = list.size() / 3;
  std::unique_ptr<uint32_t[]> trios(new uint32_t[list.size()]);
  memcpy(trios.get(), list.data(), list.size() * sizeof(uint32_t));
  std::unique_ptr<cuking_mendel_trio[]> out(new cuking_mendel_trio[num]);
  std::unique_ptr<uint64_t[]> mask(new uint64_t[num * plane]);
  std::unique_ptr<uint32_t[]> counts(new uint32_t[(size_t)64 * plane]);
  memset(out.get(), 0xAB, num * sizeof(cuking_mendel_trio));
  memset(mask.get(), 0xCD, num * plane * sizeof(uint64_t));
  memset(counts.get(), 0, (size_t)64 * plane * sizeof(uint32_t));

  if (cuking_mendel_trios_host(bits.get(), n, words, sites, trios.get(), num, out.get(),
                               with_mask ? mask.get() : nullptr) != CUKING_OK) {
    fail("the call failed", sites, 0);
    return;
  }
  std::vector<uint32_t> want_counts((size_t)64 * plane, 0);
  for (uint64_t t = 0; t < num; ++t) {
    const uint32_t c = trios[3 * t], f = trios[3 * t + 1], m = trios[3 * t + 2];
    cuking_mendel_trio want = {};
    want.child = c;
    want.father = f;
    want.mother = m;
    std::vector<uint64_t> want_mask(plane, 0);
    if (c < n)
      for (uint32_t s = 0; s < sites; ++s) {
        const uint32_t gc = code_of(bits.get() + (size_t)c * words, plane, s);
        const uint32_t gf = f < n ? code_of(bits.get() + (size_t)f * words, plane, s) : 3;
        const uint32_t gm = m < n ? code_of(bits.get() + (size_t)m * words, plane, s) : 3;
        const uint32_t code = classify(gf, gm, gc);
        if (code != 0) {
          ++want.errors[code - 1];
          want_mask[s >> 6] |= 1ull << (s & 63);
          ++want_counts[s];
        }
        want.called += gc != 3 && (f == none || gf != 3) && (m == none || gm != 3);
      }
    if (memcmp(&want, &out[t], sizeof(want)) != 0) fail("a row differs", sites, t);
    if (with_mask && memcmp(want_mask.data(), mask.get() + t * plane, plane * 8) != 0)
      fail("a mask differs", sites, t);
  }
  if (!with_mask) {
    for (uint64_t k = 0; k < num * plane; ++k)
      if (mask[k] != 0xCDCDCDCDCDCDCDCDull) fail("the mask was written", sites, k);
    return;
  }
  // the counts accumulate: the call twice is twice the counts
  for (int round = 1; round <= 2; ++round) {
    if (cuking_mendel_site_counts_host(mask.get(), num, plane, counts.get()) != CUKING_OK)
      fail("the count call failed", sites, 0);
    for (size_t s = 0; s < (size_t)64 * plane; ++s)
      if (counts[s] != (uint32_t)round * want_counts[s]) {
        fail("a site count differs", sites, s);
        break;
      }
  }
}

void check_refusals() {
  const uint32_t sites = 130, plane = 3, words = 6;
  std::unique_ptr<uint64_t[]> bits(new uint64_t[2 * words]());
  std::unique_ptr<uint32_t[]> trios(new uint32_t[3]());
  std::unique_ptr<cuking_mendel_trio[]> out(new cuking_mendel_trio[1]);
  std::unique_ptr<uint64_t[]> mask(new uint64_t[plane]());
  std::unique_ptr<uint32_t[]> counts(new uint32_t[64 * plane]());
  memset(out.get(), 0xAB, sizeof(cuking_mendel_trio));
  const cuking_status bad = CUKING_ERR_INVALID_ARGUMENT;
  expect("odd words", cuking_mendel_trios_host(bits.get(), 2, 5, sites, trios.get(), 1, out.get(),
                                               nullptr), bad);
  expect("too many sites", cuking_mendel_trios_host(bits.get(), 2, words, 193, trios.get(), 1,
                                                    out.get(), nullptr), bad);
  expect("null out", cuking_mendel_trios_host(bits.get(), 2, words, sites, trios.get(), 1, nullptr,
                                              nullptr), bad);
  expect("null trios", cuking_mendel_trios_host(bits.get(), 2, words, sites, nullptr, 1, out.get(),
                                                nullptr), bad);
  expect("null bits", cuking_mendel_trios_host(nullptr, 2, words, sites, trios.get(), 1, out.get(),
                                               nullptr), bad);
  expect("no trio", cuking_mendel_trios_host(nullptr, 2, words, sites, nullptr, 0, nullptr,
                                             nullptr), CUKING_OK);
  const unsigned char *raw = reinterpret_cast<const unsigned char *>(out.get());
  for (size_t k = 0; k < sizeof(cuking_mendel_trio); ++k)
    if (raw[k] != 0xAB) fail("a refused call wrote a row", sites, k);
  expect("no plane word", cuking_mendel_site_counts_host(mask.get(), 1, 0, counts.get()), bad);
  expect("2^32 trios", cuking_mendel_site_counts_host(mask.get(), 1ull << 32, plane, counts.get()),
         bad);
  expect("null counts", cuking_mendel_site_counts_host(mask.get(), 1, plane, nullptr), bad);
  expect("no trio to count", cuking_mendel_site_counts_host(nullptr, 0, plane, nullptr),
         CUKING_OK);
}

}  // namespace

int main() {
  check_disjoint();
  const uint32_t shapes[] = {1, 63, 64, 65, 127, 128, 4095, 4096, 4097, 64 * 64 + 65};
  for (uint32_t sites : shapes)
    for (uint32_t n : {1u, 3u, 7u}) {
      run_shape(sites, n, true);
      run_shape(sites, n, false);
    }
  run_shape(0, 3, true);
  check_refusals();
  printf("%d failures\n", g_failures);
  return g_failures != 0;
}
