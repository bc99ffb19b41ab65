// Stand-alone driver of the host side of the IBD scan of a block for the sanitizer build of
// tests/test_ibd_scan_host.py (built and run by tests/host_driver.py, csrc/king_host.cc linked in).
// Every buffer is an exact-size heap allocation, so a byte read or written past an end is caught
// -- the planes of exactly num_sites / 64 words above all: with num_sites a multiple of 64 the
// word of bit num_sites lies beyond them.
//   1. cuking_ibd_scan_host on blocks of 37 samples (one whole tile of 32 and a partial one)
//      against cuking_ibd_pairs_host over the explicit list of the block's pairs, filtered by
//      the record rule: a buffer of exactly the count, of one less (RESOURCE_EXHAUSTED, the
//      exact count, the first records) and the counting call with a null buffer;
//   2. the refusals and the calls without work.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "cuking_amd.h"
#include "host_driver_common.h"

namespace {

void run_shape(uint32_t n, uint32_t sites, bool groups, bool positions, uint32_t min_sites,
               const cuking_submatrix &block, uint64_t min_total) {
  const uint32_t plane = (sites + 63) / 64, words = 2 * plane;
  std::unique_ptr<uint64_t[]> bits(new uint64_t[(size_t)n * words]);
  // sparse breaks: mostly hom-ref / het, few hom-var, some missing; long runs exist
  for (size_t k = 0; k < (size_t)n * words; ++k) {
    const bool hom = (k / plane) & 1;
    bits[k] = hom ? next_random() & next_random() & next_random() & next_random() & next_random()
                  : next_random() & next_random();
  }
  // every third sample copies sample 0 over the middle half
  for (uint32_t c = 3; c < n; c += 3)
    for (uint32_t s = sites / 4; s < sites - sites / 4; ++s)
      for (uint32_t p = 0; p < 2; ++p) {
        const uint64_t bit = 1ull << (s & 63);
        uint64_t &to = bits[(size_t)c * words + p * plane + (s >> 6)];
        to = (to & ~bit) | (bits[p * plane + (s >> 6)] & bit);
      }
  std::unique_ptr<int32_t[]> group(new int32_t[sites]);
  std::unique_ptr<uint32_t[]> pos(new uint32_t[sites]);
  for (uint32_t s = 0; s < sites; ++s) {
    group[s] = (int32_t)(s / 300);
    const bool first = s == 0 || (groups && group[s] != group[s - 1]);
    pos[s] = first ? (uint32_t)(next_random() % 100) : pos[s - 1] + (uint32_t)(next_random() % 4);
  }
  const int32_t *g = groups ? group.get() : nullptr;
  const uint32_t *q = positions ? pos.get() : nullptr;
  const uint32_t min_length = positions ? 40 : 0;

  // the listed call over the explicit list of the block's pairs, filtered
  const bool diag = block.i_begin == block.j_begin;
  std::vector<uint32_t> list;
  for (uint32_t i = block.i_begin; i < block.i_end; ++i)
    for (uint32_t j = diag ? i + 1 : block.j_begin; j < block.j_end; ++j) {
      list.push_back(i);
      list.push_back(j);
    }
  const uint64_t num_pairs = list.size() / 2;
  std::unique_ptr<cuking_ibd_pair[]> rows(new cuking_ibd_pair[num_pairs]);
  if (cuking_ibd_pairs_host(bits.get(), n, words, sites, g, q, min_sites, min_length, list.data(),
                            num_pairs, 8, rows.get(), nullptr, 0, nullptr) != CUKING_OK)
    return fail("the listed call", sites, 0);
  std::vector<cuking_ibd_pair> want;
  for (uint64_t p = 0; p < num_pairs; ++p)
    if (rows[p].segments1 >= 1 && rows[p].length1 >= min_total) want.push_back(rows[p]);
  const uint64_t total = want.size();

  for (int mode = 0; mode < 3; ++mode) {
    // 0: exactly the count; 1: one less; 2: the counting call
    if (mode != 0 && total == 0) continue;
    const uint64_t room = mode == 0 ? total : mode == 1 ? total - 1 : 0;
    std::unique_ptr<cuking_ibd_pair[]> out(new cuking_ibd_pair[room]);
    uint64_t found = 12345;
    const cuking_status st =
        cuking_ibd_scan_host(bits.get(), n, words, sites, g, q, min_sites, min_length, &block,
                             min_total, room ? out.get() : nullptr, room, &found);
    if (st != (total > room ? CUKING_ERR_RESOURCE_EXHAUSTED : CUKING_OK))
      return fail("status", sites, (uint64_t)st * 10 + mode);
    if (found != total) return fail("count", sites, found);
    if (room && memcmp(out.get(), want.data(), room * sizeof(cuking_ibd_pair)) != 0)
      return fail("records", sites, mode);
  }
}

void run_refusals() {
  const uint32_t sites = 128, words = 4, n = 4;
  std::unique_ptr<uint64_t[]> bits(new uint64_t[n * words]());
  std::unique_ptr<uint32_t[]> pos(new uint32_t[sites]);
  for (uint32_t s = 0; s < sites; ++s) pos[s] = 10 * s;
  std::unique_ptr<cuking_ibd_pair[]> out(new cuking_ibd_pair[6]);
  uint64_t found = 0;
  const cuking_submatrix all = {0, n, 0, n}, off = {0, 2, 2, 4}, reversed = {3, 1, 3, 1},
                         overlap = {0, 3, 2, 4}, outside = {0, 5, 0, 5}, empty = {2, 2, 2, 2},
                         single = {1, 2, 1, 2};
  const cuking_status bad = CUKING_ERR_INVALID_ARGUMENT;
#define CALL(...) cuking_ibd_scan_host(__VA_ARGS__)
  expect("ok", CALL(bits.get(), n, words, sites, nullptr, pos.get(), 64, 0, &all, 0, out.get(), 6,
                    &found), CUKING_OK);  // four equal samples: six records
  if (found != 6 || out[5].sample_i != 2 || out[5].sample_j != 3 || out[0].length1 != 1270 ||
      out[0].segments2 != 1)
    fail("six records of one whole run", sites, found);
  expect("off-diagonal", CALL(bits.get(), n, words, sites, nullptr, nullptr, 64, 0, &off, 127,
                              out.get(), 4, &found), CUKING_OK);
  if (found != 4 || out[3].sample_i != 1 || out[3].sample_j != 3) fail("off", sites, found);
  expect("min_total above", CALL(bits.get(), n, words, sites, nullptr, nullptr, 64, 0, &off, 128,
                                 nullptr, 0, &found), CUKING_OK);
  if (found != 0) fail("min_total", sites, found);
  expect("null block", CALL(bits.get(), n, words, sites, nullptr, nullptr, 64, 0, nullptr, 0,
                            out.get(), 6, &found), bad);
  expect("reversed", CALL(bits.get(), n, words, sites, nullptr, nullptr, 64, 0, &reversed, 0,
                          out.get(), 6, &found), bad);
  expect("overlap", CALL(bits.get(), n, words, sites, nullptr, nullptr, 64, 0, &overlap, 0,
                         out.get(), 6, &found), bad);
  expect("outside", CALL(bits.get(), n, words, sites, nullptr, nullptr, 64, 0, &outside, 0,
                         out.get(), 6, &found), bad);
  expect("odd words", CALL(bits.get(), n, 3, sites, nullptr, nullptr, 64, 0, &all, 0, out.get(), 6,
                           &found), bad);
  expect("too many sites", CALL(bits.get(), n, words, 129, nullptr, nullptr, 64, 0, &all, 0,
                                out.get(), 6, &found), bad);
  expect("min_sites", CALL(bits.get(), n, words, sites, nullptr, nullptr, 63, 0, &all, 0,
                           out.get(), 6, &found), bad);
  expect("null count", CALL(bits.get(), n, words, sites, nullptr, nullptr, 64, 0, &all, 0,
                            out.get(), 6, nullptr), bad);
  expect("null records", CALL(bits.get(), n, words, sites, nullptr, nullptr, 64, 0, &all, 0,
                              nullptr, 6, &found), bad);
  expect("null bits", CALL(nullptr, n, words, sites, nullptr, nullptr, 64, 0, &all, 0, out.get(), 6,
                           &found), bad);
  pos[100] = 5;
  expect("decreasing pos", CALL(bits.get(), n, words, sites, nullptr, pos.get(), 64, 0, &all, 0,
                                out.get(), 6, &found), CUKING_ERR_FAILED_PRECONDITION);
  found = 9;
  expect("empty block", CALL(nullptr, n, words, sites, nullptr, nullptr, 64, 0, &empty, 0, nullptr,
                             0, &found), CUKING_OK);
  if (found != 0) fail("empty block", sites, found);
  found = 9;
  expect("1 x 1", CALL(bits.get(), n, words, sites, nullptr, nullptr, 64, 0, &single, 0, nullptr, 0,
                       &found), CUKING_OK);
  if (found != 0) fail("1 x 1", sites, found);
  found = 9;
  expect("no sites", CALL(nullptr, n, words, 0, nullptr, nullptr, 64, 0, &all, 0, nullptr, 0,
                          &found), CUKING_OK);
  if (found != 0) fail("no sites", 0, found);
#undef CALL
}

}  // namespace

int main() {
  const uint32_t n = 37;
  const cuking_submatrix blocks[] = {{0, n, 0, n}, {3, 36, 3, 36}, {0, 5, 5, n}, {2, 3, 30, n}};
  const uint32_t shapes[] = {64, 128, 1024, 1024 + 37, 4096};
  int k = 0;
  for (uint32_t sites : shapes)
    for (const cuking_submatrix &block : blocks)
      for (int variant = 0; variant < 4; ++variant, ++k)
        run_shape(n, sites, variant & 1, variant & 2, k % 2 ? 64 : 100, block,
                  k % 3 == 0 ? sites / 3 : 0);
  run_refusals();
  printf("%d failures\n", g_failures);
  return g_failures != 0;
}
